"""dwgsim_eval-hip's command line on the paths that end before a device is opened: usage, -h, bad options, -m taking an argument, and the
refusal of BAM input (no -S).  The product CLI is built by __graft_entry__.build() (make all)."""
import os, subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "dwgsim_amd", "dwgsim_eval-hip")
SAM = os.path.join(ROOT, "tests", "golden", "eval", "basic.sam")


@pytest.fixture(scope="module")
def cli():
    if not os.path.exists(CLI):
        subprocess.run(["make", "-s", "-j16", "-C", os.path.join(ROOT, "dwgsim_amd", "csrc"), "all"], check=True)
    return CLI


def run(cli, *args):
    # HIP_VISIBLE_DEVICES hides every device: a path that tried to open one would fail instead of passing by luck
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    return subprocess.run([cli, *args], capture_output=True, timeout=60, env=env)


def test_usage_without_files(cli):
    p = run(cli)
    assert p.returncode == 1 and p.stdout == b""
    e = p.stderr.decode()
    assert "Usage: dwgsim_eval-hip" in e
    for opt, default in [("-a", "[0]"), ("-d", "[1]"), ("-g", "[5]"), ("-n", "[0]"), ("-q", "[0]"), ("-s", "[-1]"), ("-e", "[-1]"),
                         ("-P", "[not using]"), ("-m", "[False]"), ("-z", "[False]"), ("-p", "[False]"), ("-i", "[False]"), ("-b", "[False]"),
                         ("-c", "[False]"), ("-S", "[False]")]:
        assert any(l.startswith("\t" + opt + "\t") and default in l for l in e.split("\n")), opt


def test_help_shows_the_parsed_values(cli):
    p = run(cli, "-a", "3", "-d", "7", "-P", "pfx", "-h")
    assert p.returncode == 1
    assert "split by [3]" in p.stderr.decode() and "factor [7]" in p.stderr.decode() and "[pfx]" in p.stderr.decode()


def test_unknown_option(cli):
    p = run(cli, "-x", SAM)
    assert p.returncode == 1 and p.stderr.decode().endswith("Unrecognized option: -?\n")


def test_missing_argument(cli):
    p = run(cli, "-S", "-a")
    assert p.returncode == 1 and "Unrecognized option: -?" in p.stderr.decode()


def test_m_consumes_an_argument(cli):
    # "m:" in the option string: the SAM path is taken as -m's argument, so no file is left and the usage is printed
    p = run(cli, "-S", "-m", SAM)
    assert p.returncode == 1 and "Usage: dwgsim_eval-hip" in p.stderr.decode()


def test_bam_is_refused(cli):
    p = run(cli, SAM)
    assert p.returncode == 1 and p.stdout == b""
    assert p.stderr == b"dwgsim_eval-hip: only SAM text is supported: pass -S (samtools view -h in.bam | dwgsim_eval-hip -S -)\n"


def test_d_zero_is_refused(cli):
    p = run(cli, "-S", "-d", "0", SAM)
    assert p.returncode == 1 and b"-d must not be 0" in p.stderr
