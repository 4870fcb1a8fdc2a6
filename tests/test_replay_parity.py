"""Replay parity on the CPU (tests/replay_common.py): the unmodified reference, its drand48() replaying the Philox stream of mode B, must
write the files the oracle writes in mode B, from exactly the draws that were dumped.  Retires "mode A == reference and mode B == same code,
other provider" as the only link between the reference and the stream the HIP kernels draw from, for every configuration without a normal.
What the reference wrote, and which stream it was fed, is recorded in tests/golden/reference_runs.json (tests/golden/make_reference_runs.py)."""
import os, random
import pytest

from replay_common import REPLAY_CASES, REPLAY_FUZZ_SEEDS, SUFFIXES, case_key, reference_run, run_mode_b, random_replay_flags, sha256


def check(oracle_bin, golden_dir, fasta, flags, tmp):
    rec = reference_run("replay", case_key(fasta, flags))
    orc, want, draws = run_mode_b(oracle_bin, os.path.join(golden_dir, fasta), flags, str(tmp))
    rrc = rec["rc"]
    if orc != 0 or rrc != 0:      # an option set both reject (the reference's own parse errors), or on which both abort the same way
        assert orc == rrc or (orc != 0 and rrc != 0), f"oracle rc {orc}, replayed reference rc {rrc}: {flags}"
        return False
    assert sha256(draws) == rec["draws_sha256"], f"mode B dumps another stream than the one the reference was fed when it was recorded: {fasta} {flags}"
    for suf in SUFFIXES:
        assert sha256(want[suf]) == rec["sha256"][suf], f"{suf} differs between the replayed reference and mode B ({len(want[suf])} bytes): {fasta} {flags}"
    assert rec["served"] == rec["avail"] == len(draws) // 8 > 0, f"the reference consumed {rec['served']} of the {len(draws) // 8} dumped draws: {fasta} {flags}"
    return True


@pytest.mark.parametrize("fasta,flags", REPLAY_CASES, ids=[f"{f}:{fl}" for f, fl in REPLAY_CASES])
def test_reference_fed_the_philox_stream_writes_mode_b(oracle_bin, golden_dir, tmp_path, fasta, flags):
    assert check(oracle_bin, golden_dir, fasta, flags, tmp_path)


@pytest.mark.parametrize("seed", REPLAY_FUZZ_SEEDS)
def test_replay_fuzz(oracle_bin, golden_dir, tmp_path, seed):
    """25 random single-end option sets per seed (Illumina / SOLiD / Ion Torrent, mutation inputs, regions)."""
    rng = random.Random(seed); ran = 0
    for k in range(25):
        fasta, flags = random_replay_flags(rng)
        d = tmp_path / f"c{k}"; d.mkdir()
        ran += bool(check(oracle_bin, golden_dir, fasta, flags, d))
    assert ran >= 15
