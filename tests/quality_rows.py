"""The quality line of k_simulate's lockstep instances (Illumina, one kernel, one output family: DT = 0, SPLIT = 0, WR = 1, 256-lane blocks) runs in the
wave's staging rows from 18 staged words per lane on (137 bases: 72 bytes; dw_simulate.hip QROWS): a Philox block's characters go down without a drain
test, and on every fourth trip the lanes with a whole unit pending take one drain together.  The cases here put the read lengths on both sides of that
edge and well past it, take the quality settings that deliver eight characters in every trip (the buffer's fullest state) and those that take the exact
fp64 try often, and compare with the oracle byte for byte -- with the row buffer ("qrows" at its default) and without it ("qrows" = 0).

tests/test_emu_quality_rows.py (CPU emulation) and tests/test_gpu_quality_rows.py (device) both run what is here; check_case takes the loaded library.
The form is forced with split = 0, writer = 1, sim_threads = 256 (2 x 600 bases would otherwise run as one-wave blocks), and every launch must report it
("sim_form")."""
import tempfile

from dwgsim_amd import api
from parity_common import compare_case, run_oracle
from sim_instances import write_fasta      # three contigs, N runs, a name longer than LDS keeps  # noqa: F401

N_PAIRS = 769      # three blocks and one lane: the last block's other lanes have no record
# read lengths of the two ends: 17 staged words (the FIFO path) | 18 words: exactly 72 bytes | ... | the headline's 150 | a second end so short that its
# record's first unit has not left when the quality line starts (its waves keep the FIFO) | ... | long reads
PAIRED = [(136, 136), (137, 137), (144, 145), (150, 150), (151, 16), (152, 153), (248, 250), (300, 600)]
SINGLE = [l1 for l1, _ in PAIRED]
PREFIXES = ["", "-P p", "-P some_prefix", "-P a_prefix_of_forty_characters_0123456789ab"]      # name lengths (and with them the record phases) spread
QUALITIES = ["", "-Q 0", "-q I", "-Q 0.3", "-Q 40"]      # -Q 0 / -q: eight characters in every trip; a large -Q: the exact quality try is taken often
FORCE = {"split": 0, "writer": 1, "sim_threads": 256}


def _cases():
    cases, k = [], 0
    for out in (1, 2):
        for l1, l2 in PAIRED:
            m = max(l1, l2)
            cases.append((2, out, f"-1 {l1} -2 {l2} -d {2 * m + 50} -s 10", k)); k += 1
        for l1 in SINGLE:
            cases.append((1, out, f"-1 {l1} -2 0", k)); k += 1
    return cases


def flags_of(case):
    lpp, out, shape, k = case
    extra = " ".join(x for x in (PREFIXES[k % len(PREFIXES)], QUALITIES[k % len(QUALITIES)]) if x)
    return f"-z {4001 + k} -N {N_PAIRS} {shape} -o {out} -e 0.01-0.03 -E 0.02 -r 0.02 -R 0.3 -X 0.5 -y 0.3 -n 5 {extra}".strip()


CASES = _cases()
CASE_IDS = [f"lpp{c[0]}-o{c[1]}-{c[2].split(' -d')[0].replace(' ', '')}" for c in CASES]
SCHEDULED = [c for c in CASES if "-1 150 " in c[2] or "-1 137 " in c[2]]      # (the emulation runs these under other schedules too)
SCHEDULED_IDS = [CASE_IDS[CASES.index(c)] for c in SCHEDULED]


def quality_line_phases(text):
    """the file offsets mod 32 at which the quality lines (the fourth of every four) of a FASTQ text start"""
    phases, at = set(), 0
    for i, line in enumerate(text.split(b"\n")[:-1]):
        if i % 4 == 3:
            phases.add(at % 32)
        at += len(line) + 1
    return phases


def check_oracle_covers_every_phase(oracle_bin, fasta, flags):
    """a case counts only if the ORACLE's text starts a quality line at each of the 32 byte phases, in every stream it writes"""
    with tempfile.TemporaryDirectory() as t:
        want = run_oracle(oracle_bin, fasta, flags, t)
    streams = [k for k in (0, 1, 2) if want[k]]
    assert streams, f"{flags}: the oracle wrote no reads"
    for k in streams:
        missing = sorted(set(range(32)) - quality_line_phases(want[k]))
        assert not missing, f"{flags}: no quality line of the oracle's stream {k} starts at offset mod 32 in {missing}"


def check_case(lib, oracle_bin, fasta, case, batch_pairs=1 << 22):
    lpp, out, _, k = case
    flags = flags_of(case)
    check_oracle_covers_every_phase(oracle_bin, fasta, flags)
    for qrows in (None, 0):      # the row buffer where the launch qualifies for it | the FIFO throughout
        opts = dict(FORCE) if qrows is None else dict(FORCE, qrows=qrows)
        try:
            res = compare_case(lib, oracle_bin, fasta, flags, batch_pairs=batch_pairs, debug_options=opts)
        except AssertionError as e:
            raise AssertionError(f"{flags} (qrows = {qrows}): {e}") from None
        ran = {api.unpack_sim_form(v) for v in res.sim_forms}
        assert ran == {(lpp, out, 0, 256, 1, 0)}, f"{flags}: the launches ran as {sorted(ran)}"
