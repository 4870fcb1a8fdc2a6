"""CPU-only check of the host code's memory ownership, on the libraries that tests/emu/build.sh and build_eval.sh build: the emulation shim
counts live hipMalloc / hipHostMalloc allocations and live streams and events, and can make the k-th allocation from a given moment fail (hip_emu.cpp
hipemu_live_allocs, hipemu_live_handles, hipemu_fail_alloc).  Every scenario must give back all it allocated and every stream and event it made -- a
context whose creation dies at its k-th allocation included; a call whose allocation fails must return an error, and the same call
repeated without the failure must then succeed and give what an undisturbed run gives.  The scenarios run in a child process: a call that
went on with a missing table crashes it.  The job level (dw_job.cpp) gets the same treatment one level up: the k-th allocation of a whole job
fails, a sink refuses its n-th call, a job is destroyed unfinished -- each must return in time with an error or the right output, and with nothing
left allocated.  Test infrastructure only."""
import os, subprocess, sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU = os.path.join(HERE, "emu")

PRELUDE = r'''
import ctypes as C, faulthandler, io, os, random, sys
faulthandler.enable()
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from dwgsim_amd import api, synth
import eval_sam

def hooks(lib):
    lib.hipemu_live_allocs.restype = C.c_long
    lib.hipemu_live_handles.restype = C.c_long
    lib.hipemu_fail_alloc.restype = C.c_long
    lib.hipemu_fail_alloc.argtypes = [C.c_long]
    return lib

lib = hooks(api.load(LIB))
elib = hooks(api.load_eval(EVAL_LIB))
FLAGS = "-z 7 -N 300 -1 50 -2 50 -d 200 -s 10 -r 0.02 -R 0.5 -X 0.3 -y 0.1"      # indels half the mutations: the walk writes insertion tables
params = api.parse_flags(FLAGS, lib)
contigs = [("c%d" % k, synth.random_contig(3000 + 700 * k, 11 + k)) for k in range(6)]
'''

DRIVER = PRELUDE + r'''
def leak_free(name, lib, fn):
    base, base_h = lib.hipemu_live_allocs(), lib.hipemu_live_handles()
    fn()
    left, left_h = lib.hipemu_live_allocs() - base, lib.hipemu_live_handles() - base_h
    assert left == 0, "%s: %d allocations left behind" % (name, left)
    assert left_h == 0, "%s: %d streams and events left behind" % (name, left_h)

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

def create_destroy(lib, create, destroy, k=0):
    """create(err) with its k-th allocation failing (0: none), then destroy -> (whether a context came back, the error code, whether the failure fired)"""
    err = C.c_int(0)
    lib.hipemu_fail_alloc(k)
    h = create(C.byref(err))
    fired = lib.hipemu_fail_alloc(0) == 0 and k > 0
    if h:
        destroy(h)
    return bool(h), err.value, fired

def failed_creates(name, lib, create, destroy):
    """a plain create / destroy, then one whose k-th allocation fails, for every k up to the allocations a create makes: an error comes back, nothing is left"""
    got = []
    leak_free(name + " create", lib, lambda: got.append(create_destroy(lib, create, destroy)))
    assert got[-1] == (True, 0, False), (name, got[-1])
    k = 1
    while True:
        leak_free("%s create, allocation %d fails" % (name, k), lib, lambda: got.append(create_destroy(lib, create, destroy, k)))
        made, code, fired = got[-1]
        if not fired:
            break
        assert not made and code < 0, "%s create: allocation %d failed, a context came back or the error code is %d" % (name, k, code)
        k += 1
    assert made and code == 0 and k > 4, (name, k, got[-1])
    print(name, "create makes", k - 1, "allocations", flush=True)

EVAL_OPTS = api.EvalOpts()
elib.dwgsim_hip_eval_opts_default(C.byref(EVAL_OPTS))
EVAL_OPTS.chunk_bytes = 4096

leak_free("context", lib, context_scenario)
leak_free("eval", elib, eval_scenario)
leak_free("job", lib, job_scenario)
failed_creates("context", lib, lambda err: lib.dwgsim_hip_create(C.byref(params), 0, err), lib.dwgsim_hip_destroy)
failed_creates("eval", elib, lambda err: elib.dwgsim_hip_eval_create(C.byref(EVAL_OPTS), 0, err), elib.dwgsim_hip_eval_destroy)
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
    base, base_h = lib.hipemu_live_allocs(), lib.hipemu_live_handles()
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
    left_h = lib.hipemu_live_handles() - base_h
    assert left_h == 0, "%s, allocation %d: %d streams and events left behind" % (stage, k, left_h)
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


JOB_DRIVER = PRELUDE + r'''
import gzip, threading
ERR_FAILED = -5      # DWGSIM_HIP_ERR_FAILED
RUN_TIMEOUT = 120    # seconds for one job; a run that takes longer hangs, and the child ends with every thread's stack on stderr
JOB = [("s%d" % k, synth.random_contig(1000 + 300 * k, 31 + k)) for k in range(3)]      # (several hundred runs of it: small)
params = api.parse_flags(FLAGS.replace("-N 300", "-N 72"), lib)
# Options that make the job a real one for the code under test: groups of at most 4000 bp -- every contig is a group of its own, three in all, so
# that the two-groups-ahead rule, the look-ahead and the recycling of the two staging buffers engage -- and a least share of one pair, so that
# every group's batches (of at most 8 pairs) are dealt to all the devices: counts are exchanged, buffers come back from other lanes.
GROUP_BP, BATCH_PAIRS, MIN_SHARE = 4000, 8, 1

class Refuse:
    # the sink callback `which` returns non-zero on its n-th call
    def __init__(self, which=None, n=0):
        self.which, self.n, self.calls, self.lock = which, n, {"mutations": 0, "reads": 0, "reads_at": 0}, threading.Lock()
    def __call__(self, which):
        with self.lock:
            self.calls[which] += 1
            return 1 if which == self.which and self.calls[which] == self.n else 0

def run(devices, offset_sink, fail_alloc=0, refuse=None, destroy_after=None, job=JOB, table_lens=None, group_bp=GROUP_BP):
    """One small job through dwgsim_hip_job_*; the fail_alloc-th allocation counted from job_create fails.
    -> (where it ended: "create" / "add_contig" / "finish" / "destroyed", or None for a complete run; the error code; the job's error text;
        the output of a complete run; allocations the failure request still waited for at the end; calls per sink callback)"""
    refuse = refuse or Refuse()
    txt, vcf, lock = bytearray(), bytearray(), threading.Lock()
    pieces = {0: [], 1: [], 2: []}
    def on_mut(user, name, t, tl, v, vl):
        if refuse("mutations"): return 1
        txt.extend(C.string_at(t, tl) if tl else b""); vcf.extend(C.string_at(v, vl) if vl else b"")
        return 0
    def on_reads(user, stream, data, n, text_n, gz):
        if refuse("reads"): return 1
        pieces[stream].append((len(pieces[stream]), bool(gz), C.string_at(data, n), text_n))
        return 0
    def on_reads_at(user, stream, offset, data, n, text_n, gz):      # (from several threads)
        if refuse("reads_at"): return 1
        with lock: pieces[stream].append((offset, bool(gz), C.string_at(data, n), text_n))
        return 0
    sink = api.JobSink(None, api.MUT_CB(on_mut), api.READS_CB(on_reads), api.MSG_CB(lambda u, m: None),
                       api.READS_AT_CB(on_reads_at) if offset_sink else api.READS_AT_CB())
    opt = api.JobOptions(1, 1, BATCH_PAIRS, group_bp, MIN_SHARE)
    err = C.c_int(0)
    devs = (C.c_int * len(devices))(*devices)
    faulthandler.dump_traceback_later(RUN_TIMEOUT, exit=True)
    base, base_h = lib.hipemu_live_allocs(), lib.hipemu_live_handles()
    lib.hipemu_fail_alloc(fail_alloc)
    where, code, text = None, 0, ""
    h = lib.dwgsim_hip_job_create(C.byref(params), devs, len(devices), C.byref(sink), C.byref(opt), C.byref(err))
    if not h:
        where, code = "create", err.value
        assert code < 0, code
    else:
        n = len(job)
        rc = lib.dwgsim_hip_job_set_contig_table(h, (C.c_char_p * n)(*[nm.encode() for nm, _ in job]), (C.c_int64 * n)(*(table_lens or [len(a) for _, a in job])), n)
        assert rc == 0, rc
        for k, (name, a) in enumerate(job):
            if k == destroy_after:
                break
            r = lib.dwgsim_hip_job_add_contig(h, name.encode(), a.ctypes.data_as(C.c_void_p), len(a))
            if r < 0 and not api.is_skip(r):
                where, code = "add_contig", r
                break
        if destroy_after is not None:
            where = "destroyed"
        else:
            rc = lib.dwgsim_hip_job_finish(h)
            if rc < 0:
                where, code = where or "finish", code or rc
                assert rc == ERR_FAILED, rc
            else:
                assert where is None, "add_contig returned %d, job_finish then %d" % (code, rc)
            text = lib.dwgsim_hip_job_last_error(h).decode(errors="replace")
        lib.dwgsim_hip_job_destroy(h)
    waiting = lib.hipemu_fail_alloc(0)
    faulthandler.cancel_dump_traceback_later()
    left = lib.hipemu_live_allocs() - base
    assert left == 0, "devices %s, allocation %d, %s: %d allocations left behind (ended at %s)" % (devices, fail_alloc, refuse.which, left, where)
    left_h = lib.hipemu_live_handles() - base_h
    assert left_h == 0, "devices %s, allocation %d, %s: %d streams and events left behind (ended at %s)" % (devices, fail_alloc, refuse.which, left_h, where)
    out = None
    if where is None:
        streams = []
        for s in range(3):
            at, blob = 0, bytearray()
            for off, gz, data, text_n in sorted(pieces[s]):
                if offset_sink:
                    assert off == at, "reads_at: stream %d has a gap or an overlap at offset %d" % (s, at)
                    at += len(data)
                piece = gzip.decompress(data) if gz else data
                assert len(piece) == text_n
                blob += piece
            streams.append(bytes(blob))
        out = (bytes(txt), bytes(vcf), streams)
    return where, code, text, out, waiting, refuse.calls

def traced(fn):
    """fn() with DWGSIM_HIP_TRACE set and stderr (the file descriptor: the library writes there) into a file -> (fn's result, the trace)"""
    import re, tempfile
    with tempfile.TemporaryFile() as f:
        sys.stderr.flush()
        saved = os.dup(2)
        os.environ["DWGSIM_HIP_TRACE"] = "1"
        os.dup2(f.fileno(), 2)
        try:
            res = fn()
        finally:
            os.dup2(saved, 2); os.close(saved)
            del os.environ["DWGSIM_HIP_TRACE"]
        f.seek(0)
        return res, f.read().decode(errors="replace")

want_one = None
for devices in ([0], [0, 0, 0]):
    for offset_sink in (False, True):
        tag = "devices %s, %s sink" % (devices, "offset" if offset_sink else "ordered")
        BIG = 1 << 40
        (where, _, _, want, waiting, calls), tr = traced(lambda: run(devices, offset_sink, fail_alloc=BIG))
        n_alloc = BIG - waiting
        # the job is what the options above are meant to make it: several groups, and batches enqueued by every device
        import re
        n_groups = len(re.findall(r"group \d+ dispatched", tr))
        busy = set(re.findall(r"dev (\d+) group \d+: batch \d+ enqueued", tr))
        assert n_groups == len(JOB) and len(busy) == len(devices), (tag, n_groups, sorted(busy), tr[-1500:])
        assert where is None and n_alloc > 10 * len(devices) and want[0] and all(want[2][:2]), (tag, where, n_alloc)
        assert want_one is None or want == want_one, tag + ": the output differs from the first job's"      # (any devices, either sink: one output)
        want_one = want
        print(tag, "makes", n_alloc, "allocations;", calls, flush=True)

        # ---- the k-th allocation of the job fails (a run takes half a second, so one device is swept with the ordered sink and three with
        # the offset sink's delivery threads: both device sets and both sink forms, every k of each) ----
        ended = {}
        for k in range(1, n_alloc + 1) if (devices == [0]) != offset_sink else ():
            where, code, text, got, waiting, _ = run(devices, offset_sink, fail_alloc=k)
            if where is None:      # (the failure was survived, or -- buffers are made as the threads' timing needs them -- this run made fewer allocations)
                assert got == want, "%s: allocation %d failed, the job completed with another output" % (tag, k)
            else:
                assert code < 0 and (where == "create" or text), (tag, k, where, code, text)
            ended[where] = ended.get(where, 0) + 1
        print(tag, "failed allocations ended at", ended, flush=True)
        assert not ended or (ended.get("create", 0) > 0 and ended.get("add_contig", 0) + ended.get("finish", 0) > 0), ended
        where, _, _, got, _, _ = run(devices, offset_sink)
        assert where is None and got == want, tag + ": a clean job after the failed ones differs from the undisturbed run"

        # ---- a sink that refuses its n-th call ----
        for which, message in (("mutations", "dwgsim-hip: the sink refused the mutation text"), ("reads_at" if offset_sink else "reads", "dwgsim-hip: writing FASTQ failed")):
            assert calls[which] > 0, (tag, calls)
            for n in range(1, calls[which] + 1):
                where, code, text, _, _, _ = run(devices, offset_sink, refuse=Refuse(which, n))
                assert where in ("add_contig", "finish") and text == message, "%s: %s refused call %d: ended at %s with %d, %r" % (tag, which, n, where, code, text)
        where, _, _, got, _, _ = run(devices, offset_sink)
        assert where is None and got == want, tag + ": a clean job after the refused ones differs from the undisturbed run"

        # ---- destroyed without finish, after 0 .. 3 contigs ----
        for k in range(len(JOB) + 1):
            where, _, _, _, _, _ = run(devices, offset_sink, destroy_after=k)
            assert where == "destroyed", (tag, k, where)

# ---- the staging grows with a group half filled (HostMem::grow keeps what is there): a contig table that understates the lengths, six
# contigs in ONE group; the same job in groups that fit what the table promised gives the same output ----
STALE = [1000] * 6
where, _, _, grown, _, _ = run([0], False, job=contigs, table_lens=STALE, group_bp=0)
where2, _, _, fitted, _, _ = run([0], False, job=contigs, table_lens=STALE)
assert where is None and where2 is None and grown == fitted and grown[0] and all(grown[2][:2]), (where, where2)
print("JOB-MEMORY-OK")
'''


def child(script, tmp_path, marker):
    for build in ("build.sh", "build_eval.sh"):
        subprocess.run([os.path.join(EMU, build)], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\nLIB = {os.path.join(EMU, 'libdwgsim_emu.so')!r}\n"
                        f"EVAL_LIB = {os.path.join(EMU, 'libdwgsim_eval_emu.so')!r}\n" + script],
                       capture_output=True, text=True, timeout=3600, cwd=str(tmp_path))
    assert r.returncode == 0 and marker in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])


def test_memory_is_owned_and_failed_allocations_leave_sound_state(tmp_path):
    child(DRIVER, tmp_path, "MEMORY-OK")


def test_job_survives_failed_allocations_refusing_sinks_and_early_destroy(tmp_path):
    child(JOB_DRIVER, tmp_path, "JOB-MEMORY-OK")
