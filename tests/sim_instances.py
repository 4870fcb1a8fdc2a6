"""Every k_simulate<LPP, OUT, DT, NTHR, WR, SPLIT> instance against the oracle, and the list of instances pinned (dw_simulate.hip DW_SIM_ALL).

tests/test_emu_sim_instances.py (CPU emulation) and tests/test_gpu_sim_instances.py (device) both run what is here; every check_* function takes the
loaded library.  The parity suites compare option sets; this module compares FORMS: each of the 66 forms the host can make of a launch (dw_host.cpp
sim_form) is forced through the debug options, run at the shapes below, compared byte for byte, and the form every launch reports ("sim_form") must be
the intended one.  A two-kernel form (l, o, d, n, w, 1) runs two instances, (l, 1, d, n, 1, 1) and (l, o, d, n, w, 2): the 66 forms cover 70 instances,
and check_every_instance_is_compared holds that set against the library's own list (dwgsim_hip_debug_sim_instances)."""
import os
import random
import subprocess

from dwgsim_amd import api, synth
from parity_common import FLOW, compare_case

ILLUMINA = "-e 0.01-0.03 -E 0.02"
SOLID = "-c 1 -e 0.02 -E 0.03"
ION = f"-c 2 -f {FLOW} -e 0.02 -E 0.03"
# (DT, NTHR, WR, split) of a form, the flags of its error model, the debug options that force it
KINDS = [
    ((0, 256, 0, 0), ILLUMINA, {"split": 0, "writer": 0}),      # one kernel, the register writer
    ((0, 256, 1, 0), ILLUMINA, {"split": 0, "writer": 1}),      # ... the FIFO writer
    ((0, 256, 0, 1), ILLUMINA, {"split": 1, "writer": 0}),      # two kernels, the second half with the register writer
    ((0, 256, 2, 1), ILLUMINA, {"split": 1, "writer": 1}),      # ... with the FIFO of 64-byte bursts
    ((0, 64, 1, 0), ILLUMINA, {"sim_threads": 64}),             # one-wave blocks, reads staged in scratch slots
    ((1, 256, 1, 0), SOLID, {}),
    ((1, 64, 1, 0), SOLID, {"sim_threads": 64}),
    ((2, 256, 1, 0), ION, {"ion_lds": 0}),                      # Ion Torrent, read buffers in scratch slots
    ((3, 256, 1, 0), ION, {"ion_lds": 1, "split": 0}),          # ... in LDS, one kernel
    ((3, 128, 1, 0), ION, {"ion_lds": 2}),                      # ... the smaller blocks
    ((3, 256, 2, 1), ION, {"ion_lds": 1}),                      # ... two kernels
]
OUT_FLAG = {1: "-o 1", 2: "-o 2", 3: "-o 0"}
# the forms, (LPP, OUT, DT, NTHR, WR, split): 11 per (LPP, OUT)
FORMS = [(lpp, out, dt, nthr, wr, split) for lpp in (2, 1) for out in (1, 2, 3) for (dt, nthr, wr, split), _, _ in KINDS]
FORM_IDS = ["%d-%d-%d-%d-%d-%d" % f for f in FORMS]
N_INSTANCES = 70

# (paired, single-end): read lengths and what goes with them
SHAPE_ONE_BASE = ("-1 1 -2 1 -d 40 -s 3", "-1 1 -2 0")
SHAPE_ION_SHORTEST = ("-1 3 -2 2 -d 40 -s 3", "-1 3 -2 0")        # the oracle, like the reference, refuses Ion Torrent reads of one base (and, for one seed, of two)
SHAPES = [
    ("-1 8 -2 7 -d 60 -s 5", "-1 8 -2 0"),                                              # the edge of one staged word
    ("-1 33 -2 31 -d 150 -s 10", "-1 33 -2 0"),                                         # around one 32-byte burst
    ("-1 64 -2 65 -d 250 -s 20", "-1 65 -2 0"),
    ("-1 129 -2 16 -d 400 -s 30 -P some_prefix", "-1 129 -2 0 -P some_prefix"),         # unequal ends; on the 200-character name, more than LDS keeps of it
    ("-1 50 -2 50 -d 200 -s 10 -y 1.0", "-1 50 -2 0 -y 1.0"),                           # every read is random
    ("-1 70 -2 40 -d 250 -s 30 -n 0 -y 0.3 -Q 4", "-1 70 -2 0 -n 0 -y 0.3 -Q 4"),       # rejections and retries on the N runs, quality noise
    ("-1 40 -2 40 -i -d 30 -s 20 -S 1 -A 1", "-1 40 -2 0 -A 2"),
]
SHAPE_ION_FLOW_WORD = ("-1 16 -2 17 -d 80 -s 5", "-1 17 -2 0")    # the flow buffers hold 16 bases per word
# -z of case k of the enumeration below is 1001 + k, except where the oracle refuses that seed's job as the reference does
SEED_BASE = 1001
SEED_CHANGED = {249: 2250}      # -z 1250, Ion Torrent -1 3 -2 2: a two-base end is one homopolymer that the flow model deletes whole, assert(0 < j) of dwgsim.c:349


def shapes_of(dt):
    return ([SHAPE_ION_SHORTEST] + SHAPES + [SHAPE_ION_FLOW_WORD]) if dt >= 2 else ([SHAPE_ONE_BASE] + SHAPES)


def pack(form):
    lpp, out, dt, nthr, wr, split = form
    return nthr << 20 | lpp << 16 | out << 12 | dt << 8 | wr << 4 | split


def instances_of(form):
    """the k_simulate instances a form runs: itself, or the two halves of the two-kernel form"""
    lpp, out, dt, nthr, wr, split = form
    return {form} if not split else {(lpp, 1, dt, nthr, 1, 1), (lpp, out, dt, nthr, wr, 2)}


def _cases():
    """form -> [(flags, debug options, batch_pairs, group_bp)].  -N 3 * NTHR + 1: three full blocks and a block of one lane; batch_pairs NTHR - 1, NTHR,
    NTHR + 1 and unbatched: a launch ends before, on and behind a block boundary and the look-back chain carries over; every third case with all contigs in one group"""
    cases, k = {}, 0
    for fi, form in enumerate(FORMS):
        lpp, out, dt, nthr, wr, split = form
        model, opts = next((m, o) for kind, m, o in KINDS if kind == (dt, nthr, wr, split))
        cases[form] = []
        for si, shape in enumerate(shapes_of(dt)):
            sh = shape[0 if lpp == 2 else 1]
            flags = f"-z {SEED_CHANGED.get(k, SEED_BASE + k)} -N {3 * nthr + 1} {sh} {OUT_FLAG[out]} {model} -r 0.02 -R 0.3 -X 0.5"
            flags += ("" if " -y " in sh else " -y 0.1") + ("" if " -n " in sh else " -n 2")
            cases[form].append((flags, dict(opts), (nthr - 1, nthr, nthr + 1, 1 << 22)[(fi + si) % 4], (1 << 30) if (fi + si) % 3 == 0 else 0))
            k += 1
    return cases


CASES = _cases()


def write_fasta(path):
    """three contigs: a (3 000 bases, six N runs of 1 ... 24 bases), ctg + 197 x (2 500, no N: a name longer than the part kept in LDS), b_with_under_scores (4 097, ten N runs)"""
    rnd = random.Random(70)

    def contig(n, runs):
        s = [rnd.choice("ACGT") for _ in range(n)]
        lens = [1, 24] + [rnd.randint(1, 24) for _ in range(runs - 2)] if runs else []
        for j, ln in enumerate(lens):      # one run per stretch of n / runs bases: they do not touch
            at = j * (n // runs) + rnd.randrange(n // runs - 25)
            s[at:at + ln] = "N" * ln
        return "".join(s)

    with open(path, "w") as f:
        for name, n, runs in (("a", 3000, 6), ("ctg" + "x" * 197, 2500, 0), ("b_with_under_scores", 4097, 10)):
            seq = contig(n, runs)
            f.write(f">{name}\n")
            for i in range(0, n, 70):
                f.write(seq[i:i + 70] + "\n")
    return str(path)


def check_form(lib, oracle_bin, fasta, form):
    """every shape of the form: all five outputs equal to the oracle's, every launch in the intended form, no Ion Torrent re-run with more room (it may change the form)"""
    for flags, opts, batch_pairs, group_bp in CASES[form]:
        what = f"form {form}: {flags} | debug options {opts} batch_pairs {batch_pairs} group_bp {group_bp}"
        try:
            res = compare_case(lib, oracle_bin, fasta, flags, batch_pairs=batch_pairs, debug_options=opts, group_bp=group_bp)
        except AssertionError as e:
            raise AssertionError(f"{what}: {e}") from None
        except subprocess.CalledProcessError as e:
            raise AssertionError(f"{what}: the oracle refused the job ({e}); give the case another seed in SEED_CHANGED") from None
        ran = {api.unpack_sim_form(v) for v in res.sim_forms}
        assert ran == {form}, f"{what}: the launches ran as {sorted(ran)}"
        assert res.flow_cap_mult == 1, f"{what}: the read capacity grew {res.flow_cap_mult}-fold"


def check_every_instance_is_compared(lib):
    """the instances the matrix runs are the instances the library has, both ways"""
    have = api.sim_instances(lib)
    assert len(set(have)) == len(have), f"listed twice: {sorted(i for i in set(have) if have.count(i) > 1)}"
    compared = set().union(*(instances_of(f) for f in FORMS))
    assert len(FORMS) == len(set(FORMS)) == 66 and all(len(c) == (9 if f[2] >= 2 else 8) for f, c in CASES.items())
    assert compared == set(have), f"k_simulate instances no form of tests/sim_instances.py runs: {sorted(set(have) - compared)}; forms without an instance: {sorted(compared - set(have))}"
    assert len(have) == N_INSTANCES


SWEEP_LENGTHS = (45, 200, 240, 800)      # two kernels by default | the register writer by LDS occupancy (200, 240) | one-wave blocks by default


def sweep_steps(data_type, ctx_index):
    """the debug overrides a context of the sweep steps through, launch by launch.  Illumina: writer x split in full, sim_threads in a Latin square over them;
    SOLiD (no writer to choose): split with sim_threads beside it; Ion Torrent: ion_lds x split in full, flow_cap and sim_threads cycling over them.  The
    context's index shifts the cycles, so the four read lengths of one (LPP, OUT) meet different combinations."""
    threads, steps = (0, 64, 256), []
    if data_type == 0:
        for wi, writer in enumerate((-1, 0, 1)):
            for si, split in enumerate((-1, 0, 1)):
                steps.append({"writer": writer, "split": split, "sim_threads": threads[(wi + si + ctx_index) % 3]})
    elif data_type == 1:
        for si, split in enumerate((-1, 0, 1)):
            steps.append({"split": split, "sim_threads": threads[(si + ctx_index) % 3]})
    else:
        for ii, ion_lds in enumerate((-1, 0, 1, 2)):
            for si, split in enumerate((-1, 0, 1)):
                steps.append({"ion_lds": ion_lds, "split": split, "flow_cap": (0, 32768)[(ii + si + ctx_index) % 2], "sim_threads": threads[(ii + 2 * si + ctx_index) % 3]})
    return steps


def check_host_asks_only_for_instances_that_exist(lib):
    """sim_form's inputs swept with launches of 4 pairs: none fails ("no k_simulate instance for this form"), every form read back runs listed instances only,
    and the sweep reaches all of them"""
    have = set(api.sim_instances(lib))
    contig = [("sweep", synth.random_contig(50000, 11))]
    seen, launches, ctx_index = set(), 0, 0
    for lpp in (2, 1):
        for out in (1, 2, 3):
            for data_type in (0, 1, 2):
                for length in SWEEP_LENGTHS:
                    flags = f"-z 7 -N 4 -1 {length} -2 {length if lpp == 2 else 0} -d {3 * length} -s 10 {OUT_FLAG[out]} -c {data_type}" + (f" -f {FLOW}" if data_type == 2 else "")
                    with api.Context(api.parse_flags(flags, lib), 0, lib) as ctx:
                        h0 = ctx.add_contigs(contig, indices=[0])
                        ctx.mutate(h0)
                        for step in sweep_steps(data_type, ctx_index):
                            for key, value in step.items():
                                ctx.debug_option(key, value)
                            try:
                                n = ctx.simulate_ranges([(h0, 0, 4)], 0, 0).n_pairs
                            except api.DwgsimError as e:
                                raise AssertionError(f"{flags} | {step}: {e}") from None
                            form = api.unpack_sim_form(ctx.debug_get("sim_form"))
                            assert n == 4 and form[0] == lpp and form[1] == out, (flags, step, form)
                            assert instances_of(form) <= have, f"{flags} | {step}: form {form} runs {sorted(instances_of(form) - have)}, which the library does not list"
                            seen |= instances_of(form)
                            launches += 1
                    ctx_index += 1
    assert launches == 24 * (9 + 3 + 12)
    assert seen == have, f"instances the sweep did not reach: {sorted(have - seen)}"
    assert len(seen) == N_INSTANCES
