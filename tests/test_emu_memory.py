"""CPU-only check of the host code's memory ownership, on the libraries that tests/emu/build.sh and build_eval.sh build: the emulation shim
counts live hipMalloc / hipHostMalloc allocations and can make the k-th allocation from a given moment fail (hip_emu.cpp hipemu_live_allocs,
hipemu_fail_alloc).  Every scenario must give back all it allocated; a call whose allocation fails must return an error, and the same call
repeated without the failure must then succeed and give what an undisturbed run gives.  The scenarios run in a child process: a call that
went on with a missing table crashes it.  Test infrastructure only."""
import os, subprocess, sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU = os.path.join(HERE, "emu")

DRIVER = r'''
import ctypes as C, faulthandler, io, os, random, sys
faulthandler.enable()
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from dwgsim_amd import api, synth
import eval_sam

def hooks(lib):
    lib.hipemu_live_allocs.restype = C.c_long
    lib.hipemu_fail_alloc.restype = C.c_long
    lib.hipemu_fail_alloc.argtypes = [C.c_long]
    return lib

lib = hooks(api.load(LIB))
elib = hooks(api.load_eval(EVAL_LIB))
FLAGS = "-z 7 -N 300 -1 50 -2 50 -d 200 -s 10 -r 0.02 -R 0.5 -X 0.3 -y 0.1"      # indels half the mutations: the walk writes insertion tables
params = api.parse_flags(FLAGS, lib)
contigs = [("c%d" % k, synth.random_contig(3000 + 700 * k, 11 + k)) for k in range(6)]

def leak_free(name, lib, fn):
    base = lib.hipemu_live_allocs()
    fn()
    left = lib.hipemu_live_allocs() - base
    assert left == 0, "%s: %d allocations left behind" % (name, left)

def context_scenario():
    ctx = api.Context(params, lib=lib)
    ids = [ctx.add_contigs([contigs[k]], first_index=k) for k in range(5)]
    for cid in ids:
        ctx.drop_contig(cid)      # five sets dropped: the pool keeps three
    ctx.debug_option("walk_cap", 4)      # the walk starts too small and runs again
    cid = ctx.add_contigs(contigs[:2])
    ctx.mutate(cid)
    ctx.mutations_text(cid)
    ctx.mutations_via_list(cid)      # mutations_take / mutlist_text / mutlist_free
    ctx.count_random(cid, 0, 200)
    ctx.set_gzip(True)
    ctx.simulate_async(cid, 0, 200, slot=0)
    b = ctx.wait(0)
    ctx.fetch(0, 0, b.bytes[0])
    ctx.fetch_gz(0, 1, b.gz_bytes[1])
    ctx.close()

def eval_scenario():
    rng = random.Random(5)
    tigs = [("chr1", 5000), ("chr2", 3000)]
    sam = eval_sam.sam_file(rng, tigs, 300)
    lines = sam.split(b"\n")
    k = next(i for i, l in enumerate(lines) if l and not l.startswith(b"@")) + 40
    lines[k] += b"\tZZ:Z:" + b"A" * 9000      # a line longer than the slots: they grow twice
    table, sm = api.eval_sam([io.BytesIO(b"\n".join(lines))], lib=elib, chunk_bytes=4096, read_bytes=1000)
    assert sm.status == 0, sm.stderr

def job_scenario():
    api.run_job_api(params, contigs[:3], devices=[0, 0, 0], batch_pairs=64, lib=lib)

leak_free("context", lib, context_scenario)
leak_free("eval", elib, eval_scenario)
leak_free("job", lib, job_scenario)
print("no leaks", flush=True)

# ---- a failed allocation in add_contigs, mutate_async or set_gzip(1), then the same call again ----
def arr(cs):
    arrs = [a for _, a in cs]
    n = len(cs)
    return (n, (C.c_char_p * n)(*[nm.encode() for nm, _ in cs]), (C.c_void_p * n)(*[a.ctypes.data for a in arrs]),
            (C.c_int64 * n)(*[len(a) for a in arrs]), (C.c_uint32 * n)(*range(n)))

ADD = arr(contigs[:2])
STAGES = ["add_contigs", "mutate_async", "set_gzip"]

def pipeline(stage=None, k=0):
    """the calls in order; at `stage` the k-th allocation fails.  Returns (outputs, whether the failure fired)"""
    base = lib.hipemu_live_allocs()
    ctx = api.Context(params, lib=lib)
    h = ctx.h
    fired = False
    def call(name, fn):
        nonlocal fired
        if name != stage:
            rc = fn()
            assert rc >= 0, (name, rc, lib.dwgsim_hip_last_error(h))
            return rc
        lib.hipemu_fail_alloc(k)
        rc = fn()
        if lib.hipemu_fail_alloc(0) > 0:      # the call made fewer than k allocations
            assert rc >= 0, (name, k, rc)
            return rc
        fired = True
        assert rc < 0, "%s: allocation %d failed, the call returned %d" % (name, k, rc)
        rc = fn()
        assert rc >= 0, "%s: allocation %d failed once, the repeated call returned %d (%s)" % (name, k, rc, lib.dwgsim_hip_last_error(h))
        return rc
    cid = call("add_contigs", lambda: lib.dwgsim_hip_add_contigs(h, *ADD))
    call("mutate_async", lambda: lib.dwgsim_hip_mutate_async(h, cid))
    call("mutate_wait", lambda: lib.dwgsim_hip_mutate_wait(h, cid))
    call("set_gzip", lambda: lib.dwgsim_hip_set_gzip(h, 1))
    out = [ctx.mutations_text(cid), ctx.mutations_text(cid + 1)]
    ctx.simulate_async(cid, 0, 200, slot=0)
    b = ctx.wait(0)
    out += [ctx.fetch(0, t, b.bytes[t]) for t in range(3)] + [ctx.fetch_gz(0, t, b.gz_bytes[t]) for t in range(3)]
    ctx.close()
    left = lib.hipemu_live_allocs() - base
    assert left == 0, "%s, allocation %d: %d allocations left behind" % (stage, k, left)
    return out, fired

want, _ = pipeline()
for stage in STAGES:
    k = 1
    while True:
        print(stage, "allocation", k, "fails", flush=True)
        got, fired = pipeline(stage, k)
        assert got == want, "%s: allocation %d failed once: the output differs from an undisturbed run's" % (stage, k)
        if not fired:
            break
        k += 1
    assert k > 1, stage
    print(stage, "made", k - 1, "allocations", flush=True)
print("MEMORY-OK")
'''


def test_memory_is_owned_and_failed_allocations_leave_sound_state(tmp_path):
    for script in ("build.sh", "build_eval.sh"):
        subprocess.run([os.path.join(EMU, script)], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\nLIB = {os.path.join(EMU, 'libdwgsim_emu.so')!r}\n"
                        f"EVAL_LIB = {os.path.join(EMU, 'libdwgsim_eval_emu.so')!r}\n" + DRIVER],
                       capture_output=True, text=True, timeout=1200, cwd=str(tmp_path))
    assert r.returncode == 0 and "MEMORY-OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
