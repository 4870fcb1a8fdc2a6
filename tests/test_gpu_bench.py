"""-m gpu: bench.py as a plain run and with --full, on the E. coli-sized workload.  A plain run prints ONE JSON line with the headline's fields
and none of the objects that only --full measures; --full still adds the legs."""
import json, os, subprocess, sys
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("host_landed", "host_landed_gz", "end_to_end", "cpu_baseline", "end_to_end_genome", "strong")


def _bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--workload", "ecoli"] + list(extra),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_and_nothing_of_full(tmp_path):
    out = _bench("--dump-outputs", str(tmp_path))
    assert out["metric"] == "M read-pairs/sec (2x150 bp PE)" and out["unit"] == "M read-pairs/s" and out["dtype"] == "u8" and out["higher_is_better"] is True
    assert out["steps"] == 3 and out["warmup"] == 1 and out["value"] > 0 and out["ms_per_step"] > 0
    assert out["config"]["pairs_per_gpu_per_step"] == 488595
    assert not set(FULL_ONLY) & set(out), sorted(set(FULL_ONLY) & set(out))
    assert {"fastq_read1.npy", "fastq_read2.npy", "launches.npy"} <= set(os.listdir(tmp_path))


def test_full_run_adds_the_legs():
    out = _bench("--full", "--no-cpu-baseline", "--no-genome-leg", "--no-strong-leg")
    assert out["value"] > 0
    for k in ("host_landed", "host_landed_gz", "end_to_end"):
        assert out[k]["value"] > 0, (k, out[k])
    assert "cpu_baseline" not in out and "end_to_end_genome" not in out and "strong" not in out
