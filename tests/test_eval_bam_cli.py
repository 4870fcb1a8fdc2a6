"""dwgsim_eval-hip's command line on BAM input, on the paths that end before or at the opening of a device (every device is hidden): input
that starts with gzip's magic is BAM and goes on to the device; text without -S still gets the message that asks for -S."""
import os, subprocess
import pytest

import bam_io as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "dwgsim_amd", "dwgsim_eval-hip")
SAM = os.path.join(ROOT, "tests", "golden", "eval", "basic.sam")
ONLY_SAM = b"dwgsim_eval-hip: only SAM text is supported: pass -S (samtools view -h in.bam | dwgsim_eval-hip -S -)\n"
NO_DEVICE = b"dwgsim_eval-hip: cannot start the evaluator on device 0"


@pytest.fixture(scope="module")
def cli():
    if not os.path.exists(CLI):
        subprocess.run(["make", "-s", "-j16", "-C", os.path.join(ROOT, "dwgsim_amd", "csrc"), "all"], check=True)
    return CLI


@pytest.fixture(scope="module")
def bam(tmp_path_factory):
    with open(SAM, "rb") as f:
        data = B.sam_to_bam(f.read())
    path = tmp_path_factory.mktemp("bam") / "basic.bam"
    path.write_bytes(data)
    return str(path), data


def run(cli, *args, stdin=b""):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    return subprocess.run([cli, *args], input=stdin, capture_output=True, timeout=60, env=env)


def test_bam_file_goes_to_the_device(cli, bam):
    p = run(cli, bam[0])
    assert p.returncode == 1 and p.stdout == b""
    assert b"only SAM text" not in p.stderr and p.stderr.startswith(NO_DEVICE)


def test_bam_on_stdin_goes_to_the_device(cli, bam):
    p = run(cli, "-p", bam[0], "-", stdin=bam[1])
    assert p.returncode == 1 and p.stdout == b"" and p.stderr.startswith(NO_DEVICE)


def test_text_file_without_S_is_refused(cli, bam):
    for args in ([SAM], [bam[0], SAM], [SAM, bam[0]]):
        p = run(cli, *args)
        assert p.returncode == 1 and p.stdout == b"" and p.stderr == ONLY_SAM, args


def test_text_on_stdin_without_S_is_refused(cli, bam):
    with open(SAM, "rb") as f:
        text = f.read()
    for args, stdin in (["-"], text), ([bam[0], "-"], text), (["-"], b""), (["-"], b"\x1f"):
        p = run(cli, *args, stdin=stdin)
        assert p.returncode == 1 and p.stdout == b"" and p.stderr == ONLY_SAM, args


def test_usage_says_bam_is_the_default(cli):
    p = run(cli)
    assert any(l.startswith("\t-S\t") and "input is SAM (default: BAM)" in l and "[False]" in l for l in p.stderr.decode().split("\n"))
