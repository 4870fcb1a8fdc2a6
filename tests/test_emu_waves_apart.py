"""CPU-only: the kernels under a schedule where the waves of a block run APART (tests/emu/hip_emu.cpp HIPEMU_WAVES_APART): one wave alone until each of
its lanes has finished or waits at __syncthreads(), the last wave first -- a legal GPU schedule, since waves are unordered between barriers -- with LDS
poisoned at every block start.  In the default round-robin schedule every wave finishes a table fill before any wave passes its first wave operation,
and static __shared__ storage keeps the previous block's table, so a missing barrier between a fill and its first use never shows; here it shows every
time.  Every case must equal the oracle (or the eval model) byte for byte.

Found by this file: k_simulate's first half (SPLIT = 1, Illumina) read the log2 table s_lg of its error-site gaps with no barrier behind the fill
(test_short_illumina_reads_with_errors[split=1-...] failed until dw_simulate.hip got one)."""
import io, os, random, subprocess
import pytest

from dwgsim_amd import api
from parity_common import compare_case

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.run([os.path.join(HERE, "emu", "build.sh")], check=True, stdout=subprocess.DEVNULL)
    return api.load(os.path.join(HERE, "emu", "libdwgsim_emu.so"))


@pytest.fixture(autouse=True)
def waves_apart(monkeypatch):
    monkeypatch.setenv("HIPEMU_WAVES_APART", "all")
    monkeypatch.delenv("HIPEMU_WAVES_SEED", raising=False)


ILLUMINA = [
    ("tiny.fa", "-z 9 -N 700 -1 50 -2 40 -e 0.02 -E 0.01"),                           # <= 50 bp: the host picks the two-kernel form by default
    ("tiny.fa", "-z 10 -N 600 -1 36 -2 50 -e 0.001-0.05 -E 0.01-0.03 -r 0.01"),        # an error ramp: sites thinned per position
    ("odd.fa", "-z 3 -N 500 -1 50 -2 50 -d 200 -s 20 -r 0.1 -R 1.0 -X 0.7 -n 50 -e 0.03"),
    ("ex1.fa", "-z 13 -N 600 -e 0.01 -E 0.02"),
]


@pytest.mark.parametrize("split", [1, 0], ids=["split=1", "split=0"])
@pytest.mark.parametrize("fasta,flags", ILLUMINA, ids=[f"{f}:{fl}" for f, fl in ILLUMINA])
def test_short_illumina_reads_with_errors(emu_lib, oracle_bin, golden_dir, fasta, flags, split):
    compare_case(emu_lib, oracle_bin, os.path.join(golden_dir, fasta), flags, batch_pairs=333, debug_options={"split": split})


def test_a_shuffled_wave_order(emu_lib, oracle_bin, golden_dir, monkeypatch):
    """HIPEMU_WAVES_SEED: the waves of each block in an order of their own"""
    for seed in ("1", "7"):
        monkeypatch.setenv("HIPEMU_WAVES_SEED", seed)
        for split in (1, 0):
            compare_case(emu_lib, oracle_bin, os.path.join(golden_dir, "tiny.fa"), "-z 9 -N 500 -1 50 -2 40 -e 0.02 -E 0.01 -r 0.02", batch_pairs=250, debug_options={"split": split})


def test_solid(emu_lib, oracle_bin, golden_dir):
    compare_case(emu_lib, oracle_bin, os.path.join(golden_dir, "tiny.fa"), "-z 8 -N 700 -c 1 -1 50 -2 35 -d 300 -r 0.02 -R 0.5 -e 0.05 -E 0.03 -y 0.1", batch_pairs=333)


@pytest.mark.parametrize("home", [{"ion_lds": 1}, {"ion_lds": 1, "split": 0}], ids=["two-kernels", "one-kernel"])
@pytest.mark.parametrize("flags", [
    "-z 9 -N 400 -c 2 -f TACGTACGTCTGAGCATCGATCGATGTACAGC -1 100 -2 0 -e 0.05 -y 0.1",
    "-z 9 -N 300 -c 2 -f TACG -1 100 -2 60 -e 0.2 -E 0.1 -d 300 -o 0",
])
def test_ion_torrent_buffers_in_lds(emu_lib, oracle_bin, golden_dir, flags, home):
    compare_case(emu_lib, oracle_bin, os.path.join(golden_dir, "tiny.fa"), flags, batch_pairs=300, debug_options=home)


@pytest.mark.parametrize("opts", [{"site_slots": 0}, {"site_slots": 1}, {"site_slots": 1, "site_slot_cap": 3}], ids=["look-back", "slots", "slot-outgrown"])
def test_dense_walk_and_both_forms_of_the_site_scan(emu_lib, oracle_bin, golden_dir, opts):
    compare_case(emu_lib, oracle_bin, os.path.join(golden_dir, "tiny.fa"), "-z 4 -N 600 -r 0.1 -R 0.5 -I 3 -X 0.6 -e 0.01", batch_pairs=700, debug_options=opts)


def test_gzip_members_made_by_the_kernels(emu_lib, golden_dir):
    from parity_common import check_gpu_gzip
    check_gpu_gzip(emu_lib, os.path.join(golden_dir, "tiny.fa"), "-z 9 -N 600 -1 70 -2 50 -r 0.01 -y 0.1", sizes=(250, 1))


def test_eval_kernels():
    import eval_model as M
    import eval_sam as S
    subprocess.run([os.path.join(HERE, "emu", "build_eval.sh")], check=True, stdout=subprocess.DEVNULL)
    lib = api.load_eval(os.path.join(HERE, "emu", "libdwgsim_eval_emu.so"))
    rng = random.Random(5)
    sam = S.sam_file(rng, [("chr1", 5000), ("chr10", 3000)], 900)
    for o in ({}, {"a": 3, "m": 1, "p": 1}):
        want = M.run([sam], M.Opts(**o))
        table, sm = api.eval_sam([io.BytesIO(sam)], lib=lib, chunk_bytes=4096, read_bytes=1000, **o)
        assert sm.status == want.status and sm.stderr == want.stderr
        assert table == want.table and sm.incorrect == want.incorrect and sm.n == want.n
