"""The sequence line of k_simulate's FIFO instances (Illumina, one kernel, one output family: DT = 0, SPLIT = 0, WR = 1, 256-lane blocks) leaves in
lockstep 32-byte units cut at each lane's own destination (dw_simulate.hip SEQ_LOCKSTEP): a head that fills the pending unit, whole units from
registers, a tail.  The cases here put read lengths on every edge of that cut and record starts on every byte phase, and compare with the oracle byte
for byte.

tests/test_emu_text_bursts.py (CPU emulation) and tests/test_gpu_text_bursts.py (device) both run what is here; check_case takes the loaded library.
The form is forced with split = 0, writer = 1, and every launch must report it ("sim_form")."""
import tempfile

from dwgsim_amd import api
from parity_common import compare_case, run_oracle
from sim_instances import write_fasta      # three contigs, N runs, a name longer than LDS keeps  # noqa: F401

N_PAIRS = 769      # three blocks and one lane
# read lengths of the two ends: 1 | around one, two, three units | the edge at which 72 bytes of staged bases per lane are first reached (18 words: 137 bases)
# | the headline's 150 | unequal ends | a long read
PAIRED = [(1, 1), (31, 32), (33, 63), (64, 65), (95, 97), (136, 137), (150, 150), (151, 16), (248, 248)]
SINGLE = [1, 31, 32, 33, 63, 64, 65, 95, 97, 136, 137, 150, 151, 248]
PREFIXES = ["", "-P p", "-P some_prefix", "-P a_prefix_of_forty_characters_0123456789ab"]      # name lengths (and with them the record phases) spread
QUALITIES = ["", "-Q 0", "-q I", "-Q 40", "-Q 4"]      # -Q 0 / -q: no draws; a large -Q: the exact quality try is taken more often
FORCE = {"split": 0, "writer": 1}


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
    return f"-z {3001 + k} -N {N_PAIRS} {shape} -o {out} -e 0.01-0.03 -E 0.02 -r 0.02 -R 0.3 -X 0.5 -y 0.3 -n 5 {extra}".strip()


CASES = _cases()
CASE_IDS = [f"lpp{c[0]}-o{c[1]}-{c[2].split(' -d')[0].replace(' ', '')}" for c in CASES]
HEADLINE = [c for c in CASES if "-1 150 " in c[2]]      # (the emulation runs these under other schedules too)
HEADLINE_IDS = [CASE_IDS[CASES.index(c)] for c in HEADLINE]


def sequence_line_phases(text):
    """the file offsets mod 32 at which the sequence lines (the second of every four) of a FASTQ text start"""
    phases, at = set(), 0
    for i, line in enumerate(text.split(b"\n")[:-1]):
        if i % 4 == 1:
            phases.add(at % 32)
        at += len(line) + 1
    return phases


def check_oracle_covers_every_phase(oracle_bin, fasta, flags):
    """a case counts only if the ORACLE's text starts a sequence line at each of the 32 byte phases, in every stream it writes"""
    with tempfile.TemporaryDirectory() as t:
        want = run_oracle(oracle_bin, fasta, flags, t)
    streams = [k for k in (0, 1, 2) if want[k]]
    assert streams, f"{flags}: the oracle wrote no reads"
    for k in streams:
        missing = sorted(set(range(32)) - sequence_line_phases(want[k]))
        assert not missing, f"{flags}: no sequence line of the oracle's stream {k} starts at offset mod 32 in {missing}"


def check_case(lib, oracle_bin, fasta, case, batch_pairs=1 << 22):
    lpp, out, _, k = case
    flags = flags_of(case)
    check_oracle_covers_every_phase(oracle_bin, fasta, flags)
    try:
        res = compare_case(lib, oracle_bin, fasta, flags, batch_pairs=batch_pairs, debug_options=dict(FORCE))
    except AssertionError as e:
        raise AssertionError(f"{flags}: {e}") from None
    ran = {api.unpack_sim_form(v) for v in res.sim_forms}
    assert ran == {(lpp, out, 0, 256, 1, 0)}, f"{flags}: the launches ran as {sorted(ran)}"
