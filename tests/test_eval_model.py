"""The plain-Python model of dwgsim_eval (tests/eval_model.py) against hand-worked answers for the SAM fixtures in tests/golden/eval.
Every expected count below was worked out by reading the fixture's records (comments give the reasoning); the model has to reproduce them.
The GPU evaluator and its CPU emulation are then held to the model (tests/test_eval_emu.py, tests/test_gpu_eval.py)."""
# The model's own anchor is no longer these fixtures alone: tests/test_eval_reference.py holds it (and the kernels) to the recorded answers of
# the unmodified reference evaluator (tests/golden/eval_reference_runs.json).
import os
import pytest

import eval_model as M

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval")
MC, MI, MU, UM, UU = range(5)


def fx(name):
    with open(os.path.join(GOLD, name), "rb") as f:
        return f.read()


def run(names, **o):
    if "P" in o and isinstance(o["P"], str):
        o["P"] = o["P"].encode()
    return M.run([fx(n) for n in ([names] if isinstance(names, str) else names)], M.Opts(**o))


def h(**bins):
    """hist from keyword bins: s60=(mc, mi, mu, um, uu), m5000 = score -5000"""
    out = {}
    for k, v in bins.items():
        out[(-1 if k[0] == "m" else 1) * int(k[1:])] = list(v)
    return out


def rows(res):
    return [l for l in res.table.decode().split("\n") if l and not l.startswith("#")]


def test_basic_table_rows_by_hand():
    # pair 0: R1 at POS 101 = name pos 100 (mc, MAPQ 60); R2 reverse strand as the name says (mc, 30)
    # pair 1: R1 at 507 -> 506 vs 500: 6 > -g 5 (mi, 20); R2 unmapped (mu, MAPQ 0)
    # pair 2: random: R1 mapped (um, 10), R2 unmapped (uu, 0)
    r = run("basic.sam")
    assert r.status == 0 and r.n == 3
    assert r.hist == h(s60=(1, 0, 0, 0, 0), s30=(1, 0, 0, 0, 0), s20=(0, 1, 0, 0, 0), s10=(0, 0, 0, 1, 0), s0=(0, 0, 1, 0, 1))
    t = r.table.decode().split("\n")
    assert t[0] == "# thr | the minimum mapping quality threshold"
    assert sum(1 for l in t if l.startswith("#")) == 19
    rr = rows(r)
    assert len(rr) == 61          # 60 down to 0, empty bins printed; 6 records -> field width 1
    assert rr[0] == "60 1 0 0 0 0 1 1 0 0 0 0 1 1.000e+00 1.000e+00 0.000e+00 2.500e-01 1.000e+00 0.000e+00"
    assert rr[1] == "59 0 0 0 0 0 0 1 0 0 0 0 1 0.000e+00 0.000e+00 0.000e+00 2.500e-01 1.000e+00 0.000e+00"
    assert rr[40] == "20 0 1 0 0 0 1 2 1 0 0 0 3 0.000e+00 0.000e+00 0.000e+00 5.000e-01 6.667e-01 0.000e+00"
    assert rr[50] == "10 0 0 0 1 0 1 2 1 0 1 0 4 0.000e+00 0.000e+00 1.000e+00 5.000e-01 6.667e-01 5.000e-01"
    assert rr[60] == "00 0 0 1 0 1 2 2 1 1 1 1 6 0.000e+00 0.000e+00 0.000e+00 5.000e-01 6.667e-01 5.000e-01"
    assert r.stderr == b"Analyzing...\nCurrently on:\n0\r3\nAnalysis complete.\n"


def test_d_divides_mapq_twice():
    # -a 0 -d 3: 60 / 3 = 20, capped at 255, / 3 again = 6, printed 6 * 3 = 18 (a single division would print 60)
    r = run("basic.sam", d=3)
    assert r.hist == h(s6=(1, 0, 0, 0, 0), s3=(1, 0, 0, 0, 0), s2=(0, 1, 0, 0, 0), s1=(0, 0, 0, 1, 0), s0=(0, 0, 1, 0, 1))
    assert [l.split()[0] for l in rows(r)] == ["18", "15", "12", "09", "06", "03", "00"]


def test_clips_and_the_g_boundary():
    # name pos 200 everywhere; left = POS - 1 - leading S/H: 3S at 204 -> 200 (0); 2H3S at 207 -> 201 (1); 2H3S at 208 -> 202 (2);
    # 50M at 196 -> 195 (5 = g: correct); 50M at 195 -> 194 (6 = g + 1: incorrect); 3M2S at 201 -> 200 (trailing clips do not count)
    assert run("clips.sam").hist == h(s40=(5, 1, 0, 0, 0))
    assert run("clips.sam", g=0).hist == h(s40=(2, 4, 0, 0, 0))
    assert run("clips.sam", g=1).hist == h(s40=(3, 3, 0, 0, 0))
    assert run("clips.sam", g=6).hist == h(s40=(6, 0, 0, 0, 0))


def test_filters_read_end_one_counts_and_i_has_priority():
    # pair 0: end 1 (err, sub, indel) = (2, 1, 0), end 2 = (0, 0, 1); pair 1: end 1 = (1, 0, 1), end 2 = (3, 2, 0); MAPQs 50 40 30 20
    assert run("filters.sam", e=2).hist == h(s50=(1, 0, 0, 0, 0), s40=(1, 0, 0, 0, 0))      # read 2 of pair 0 kept on end 1's count
    assert run("filters.sam", e=0).hist == {}                                                # ... and nothing on end 2's
    assert run("filters.sam", s=1).hist == h(s50=(1, 0, 0, 0, 0), s40=(1, 0, 0, 0, 0))
    assert run("filters.sam", s=0).hist == h(s30=(1, 0, 0, 0, 0), s20=(1, 0, 0, 0, 0))
    ind = h(s40=(1, 0, 0, 0, 0), s30=(1, 0, 0, 0, 0))                                        # -i: each end's own indel count
    assert run("filters.sam", i=1).hist == ind
    assert run("filters.sam", i=1, e=2).hist == ind                                          # -i wins over -e
    assert run("filters.sam", e=2, s=0).hist == {}                                           # -e passes pair 0, then -s (sub 1 != 0) drops it
    assert run("filters.sam", e=2, s=1).hist == h(s50=(1, 0, 0, 0, 0), s40=(1, 0, 0, 0, 0))
    assert run("filters.sam", i=1, s=5).hist == ind                                          # with -i neither -e nor -s is looked at
    assert run("filters.sam", e=2, b=1, c=1).table == run("filters.sam", e=2).table          # -b -c swap counts nobody reads
    assert all(run("filters.sam", **o).n == 2 for o in ({"e": 0}, {"i": 1}, {"s": 0}))       # filters do not change n


def test_m_skips_repeats_of_the_record_before():
    # 0 m0/R1 mc 60 | 1, 2 m0/R1 again: skipped | 3 m0/R2 mc 50 | 4 m0/R2 again: skipped | 5 m1/R1 mc 40 | 6 m0/R1 after m1: not a repeat,
    # mc 9 | 7 m1/R2 mc 40
    r = run("multi.sam", m=1)
    assert r.hist == h(s60=(1, 0, 0, 0, 0), s50=(1, 0, 0, 0, 0), s40=(2, 0, 0, 0, 0), s9=(1, 0, 0, 0, 0)) and r.n == 3
    # without -m: record 1 on chr2 and record 2 at 900 are mi at 3, record 4 at 500 is mi at 7; n counts five READ1 records
    r = run("multi.sam")
    assert r.hist == h(s60=(1, 0, 0, 0, 0), s50=(1, 0, 0, 0, 0), s40=(2, 0, 0, 0, 0), s9=(1, 0, 0, 0, 0), s7=(0, 1, 0, 0, 0), s3=(0, 2, 0, 0, 0))
    assert r.n == 5


def test_m_carries_across_files():
    data = fx("multi.sam")
    head, body = M.split_header(data)
    lines = body.split(b"\n")
    a = head + b"\n".join(lines[:2]) + b"\n"            # records 0, 1 | 2.. : record 2 repeats record 1 across the file boundary
    b = head + b"\n".join(lines[2:])
    assert M.run([a, b], M.Opts(m=1)).hist == run("multi.sam", m=1).hist


def test_contig_existence_is_a_prefix_match():
    # header: chr1 only.  "chr10 ..." starts with chr1: accepted.  Mapped to chr1: mi (exact compare); RNAME chr10 is no @SQ: mi.
    # the random pair names chr3 but is not checked: um at 5; its R2 has RNAME * without FLAG 0x4, so it counts as mapped: um at 0
    r = run("prefix_ok.sam")
    assert r.status == 0 and r.hist == h(s30=(0, 2, 0, 0, 0), s5=(0, 0, 0, 1, 0), s0=(0, 0, 0, 1, 0))
    r = run("prefix_missing.sam")
    assert (r.status, r.error_code, r.error_record) == (1, M.E_CONTIG, 1) and r.table == b""
    assert b"Variable/Value: chr3 100 100 0 0 0 0 0 0 0 0 0 0 1.\n" in r.stderr
    assert b"the mapped contig does not exist in the SAM header; perhaps you have a read name prefix?" in r.stderr


def test_read_name_prefix():
    # -P run7: "run7_" is dropped.  Pair 1: R1 reverse as named (mc); R2 forward but named reverse (mi)
    r = run("readprefix.sam", P="run7")
    assert r.hist == h(s60=(3, 1, 0, 0, 0)) and r.n == 2
    r = run("readprefix.sam")                 # no -P: "run7_chr1" is no contig
    assert (r.error_code, r.error_record) == (M.E_CONTIG, 0)
    r = run("readprefix.sam", P="run8")
    assert (r.error_code, r.error_record) == (M.E_PREFIX, 0)
    assert b'In function "process_bam": Fatal Error[OutOfRange]. Variable/Value: run7_chr1 100 100 0 0 0 0 0 0 0 0 0 0 0.\n' in r.stderr
    r = run("readprefix.sam", P="run")        # prefix + ONE character dropped: "_chr1 ..." is left
    assert r.error_code == M.E_CONTIG and b"Variable/Value: _chr1 100 100" in r.stderr


def test_alignment_scores():
    # s0: AS 10 XS 30 | XS 5 AS 5;  s1: AS:f (counts 0) XS -3 | AS 12, no XS;  s2: MAPQ 0 | unmapped;  s3: AS -7 XS:Z | AS 4294967295 (-1) XS -1
    r = run("scores.sam", a=3)
    assert r.hist == {3: [1, 0, 0, 0, 0], 0: [2, 0, 0, 0, 0], -7: [1, 0, 0, 0, 0], -20: [1, 0, 0, 0, 0], -5000: [2, 0, 1, 0, 0]}
    assert len(rows(r)) == 3 + 5000 + 1 and rows(r)[0].startswith("03 ") and rows(r)[-1].startswith("-5000 ")
    assert run("scores.sam", a=1).hist == {10: [1, 0, 0, 0, 0], 5: [1, 0, 0, 0, 0], 0: [1, 0, 0, 0, 0], 12: [1, 0, 0, 0, 0],
                                           -5000: [1, 0, 1, 0, 0], -7: [1, 0, 0, 0, 0], -1: [1, 0, 0, 0, 0]}
    assert run("scores.sam", a=2).hist == {30: [1, 0, 0, 0, 0], 5: [1, 0, 0, 0, 0], -3: [1, 0, 0, 0, 0], -5000: [2, 0, 1, 0, 0],
                                           0: [1, 0, 0, 0, 0], -1: [1, 0, 0, 0, 0]}
    # -d 3: C truncation, the floor stays -5000 / 3 = -1666 (printed -4998)
    r = run("scores.sam", a=3, d=3)
    assert r.hist == {1: [1, 0, 0, 0, 0], 0: [2, 0, 0, 0, 0], -2: [1, 0, 0, 0, 0], -6: [1, 0, 0, 0, 0], -1666: [2, 0, 1, 0, 0]}
    assert rows(r)[0].startswith("03 ") and rows(r)[-1].startswith("-4998 ")


def test_score_zero_is_always_in_the_range():
    # only the record with AS 10, XS 30 (-20): rows still start at 0
    head, body = M.split_header(fx("scores.sam"))
    rr = rows(M.run([head + body.split(b"\n")[0] + b"\n"], M.Opts(a=3)))
    assert rr[0] == "00 0 0 0 0 0 0 0 0 0 0 0 0 0.000e+00 0.000e+00 0.000e+00 0.000e+00 0.000e+00 0.000e+00"
    assert rr[-1] == "-20 1 0 0 0 0 1 1 0 0 0 0 1 1.000e+00 1.000e+00 0.000e+00 1.000e+00 1.000e+00 0.000e+00" and len(rr) == 21


def test_random_reads_go_to_um_and_uu():
    r = run("basic.sam")
    assert r.hist[10][UM] == 1 and r.hist[0][UU] == 1
    assert sum(v[UM] + v[UU] for v in r.hist.values()) == 2


def test_single_end_q_and_z():
    # -z: mc 60; reverse strand named forward: mi at 2; unmapped: mu at 0
    r = run("single.sam", z=1)
    assert r.hist == h(s60=(1, 0, 0, 0, 0), s2=(0, 1, 0, 0, 0), s0=(0, 0, 1, 0, 0)) and r.n == 3
    r = run("single.sam", z=1, q=10)           # below -q: out of the table, still in n
    assert r.hist == h(s60=(1, 0, 0, 0, 0)) and r.n == 3
    r = run("single.sam")
    assert (r.error_code, r.error_record) == (M.E_NOT_PAIRED, 0)
    assert r.stderr.endswith(b'\rIn function "run": Fatal Error[OutOfRange]. Message: Found a read that was not paired.\n'
                             b" ***** Exiting due to errors *****\n" + M.BREAK.encode())
    r = run("basic.sam", z=1, q=61)            # every record is below -q, and still the first is checked against -z
    assert (r.error_code, r.error_record) == (M.E_PAIRED, 0) and b"Found a read that was paired end" in r.stderr


def test_fatal_errors_first_record_decides():
    r = run("err_name.sam")
    assert (r.status, r.error_code, r.error_record) == (1, M.E_NAME, 1)
    assert b"Variable/Value: not_a_dwgsim read.\nMessage: [dwgsim_eval] read was not generated by dwgsim?.\n" in r.stderr
    assert r.stdout == b""
    r = run("err_lowq_name.sam", q=10)         # MAPQ below -q: the name is never read
    assert r.status == 0 and r.n == 1 and r.hist == h(s60=(2, 0, 0, 0, 0))
    assert run("err_lowq_name.sam").error_record == 1
    r = run("err_single.sam")                  # record 2 is single-end (record 3 is also no dwgsim name, but later)
    assert (r.error_code, r.error_record) == (M.E_NOT_PAIRED, 2)
    assert (run("err_single.sam", z=1).error_code, run("err_single.sam", z=1).error_record) == (M.E_PAIRED, 0)
    r = run("err_malformed.sam")
    assert (r.error_code, r.error_record) == (M.E_MALFORMED, 1)
    r = run(["basic.sam", "err_name.sam"])     # record indices run across files
    assert (r.error_code, r.error_record) == (M.E_NAME, 7)


def test_n_warning():
    r = run("basic.sam", n=5)
    assert r.stderr == (b"Analyzing...\nCurrently on:\n0\r3\n(-n)=5\tn=3\n" + M.BREAK.encode() +
                        b'\rIn function "run": Warning[OutOfRange]. Message: Number of reads found differs from the number specified (-n).\n'
                        b" ***** Warning *****\n" + M.BREAK.encode() + b"Analysis complete.\n")
    assert r.table == run("basic.sam").table
    assert b"(-n)" not in run("basic.sam", n=3).stderr


def test_p_prints_header_and_incorrect_records_verbatim():
    r = run(["basic.sam", "clips.sam"], p=1)
    head, body = M.split_header(fx("basic.sam"))
    lines = body.split(b"\n")
    cl = M.split_header(fx("clips.sam"))[1].split(b"\n")
    assert r.incorrect == head + lines[2] + b"\n" + lines[4] + b"\n" + cl[4] + b"\n"       # mi of basic, um of basic, mi of clips
    assert r.stdout == r.incorrect + r.table


def test_empty_input_prints_one_zero_row():
    r = run("empty.sam")
    assert r.status == 0 and r.n == 0
    assert rows(r) == ["00 0 0 0 0 0 0 0 0 0 0 0 0 0.000e+00 0.000e+00 0.000e+00 0.000e+00 0.000e+00 0.000e+00"]


def test_wide_field_width():
    # 1 + log10(total): 12 records -> width 2
    r = run(["basic.sam", "basic.sam"])
    assert rows(r)[0] == "60  2  0  0  0  0  2  2  0  0  0  0  2 1.000e+00 1.000e+00 0.000e+00 2.500e-01 1.000e+00 0.000e+00"


@pytest.mark.parametrize("bad_d", [0])
def test_d_zero_is_refused(bad_d):
    with pytest.raises(ValueError):
        run("basic.sam", d=bad_d)
