#!/usr/bin/env python3
"""Record what the UNMODIFIED reference (oracle/_ref/dwgsim, built by oracle/Makefile where the reference sources are present) answers on the
cases of three test modules, into tests/golden/reference_runs.json, so that those tests run without the reference:
  cli     tests/test_cli_surface.py: exit code and stderr lines on every bad command line
  replay  tests/test_replay_parity.py, tests/test_gpu_parity.py: the reference with its drand48() replaying the Philox stream of mode B --
          exit code, draws served / available, sha256 of the stream it was fed and of its five outputs (FASTQ after gunzip)
  mode_a  tests/test_oracle_mode_a_fuzz.py: exit code and sha256 of the five outputs on every random option set

usage: python tests/golden/make_reference_runs.py   (writes reference_runs.json)"""
import json, os, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from replay_common import REF_BIN, REPLAY_CASES, REPLAY_FUZZ_SEEDS, case_key, random_replay_flags, run_replay, sha256
import test_cli_surface, test_oracle_mode_a_fuzz


def main():
    if not os.path.exists(REF_BIN):
        raise SystemExit(f"{REF_BIN} is missing: build it with `make -C oracle ref` where the reference sources are present")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "oracle"], check=True)
    oracle = os.path.join(ROOT, "oracle", "build", "dwgsim_oracle")
    runs = {"reference": "nh13/DWGSIM v0.1.17-dev (src/*.c compiled unmodified, oracle/Makefile)", "cli": {}, "replay": {}, "mode_a": {}}
    with tempfile.TemporaryDirectory() as t, ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        for k, args in enumerate(test_cli_surface.BAD):
            d = os.path.join(t, f"cli{k}"); os.makedirs(d)
            rc, lines = test_cli_surface.said(REF_BIN, args, d)
            runs["cli"][test_cli_surface.case_id(args)] = {"rc": rc, "lines": lines}

        import random
        replay = list(REPLAY_CASES)
        for seed in REPLAY_FUZZ_SEEDS:
            rng = random.Random(seed)
            replay += [random_replay_flags(rng) for _ in range(25)]

        def one_replay(k):
            fasta, flags = replay[k]
            d = os.path.join(t, f"replay{k}"); os.makedirs(d)
            rc, out, served, avail, draws = run_replay(oracle, os.path.join(HERE, fasta), flags, d)
            return case_key(fasta, flags), {"rc": rc, "served": served, "avail": avail, "draws_sha256": sha256(draws),
                                            "sha256": {suf: sha256(b) for suf, b in out.items()}}
        runs["replay"] = dict(ex.map(one_replay, range(len(replay))))

        mode_a = []
        for seed, count, inputs in test_oracle_mode_a_fuzz.FUZZ_SETS:
            mode_a += test_oracle_mode_a_fuzz.option_sets(HERE, seed, count, inputs)[0]

        def one_mode_a(k):
            _, fasta, flags = mode_a[k]
            rc, out = test_oracle_mode_a_fuzz.run_mode_a([REF_BIN], fasta, flags, os.path.join(t, f"a{k}"), True)
            return case_key(fasta, flags), {"rc": rc, "sha256": out}
        runs["mode_a"] = dict(ex.map(one_mode_a, range(len(mode_a))))
    with open(os.path.join(HERE, "reference_runs.json"), "w") as f:
        json.dump(runs, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"reference_runs.json: {len(runs['cli'])} command lines, {len(runs['replay'])} replayed option sets, {len(runs['mode_a'])} mode A option sets")


if __name__ == "__main__":
    main()
