"""Throughput of dwgsim_eval-hip (not part of bench.py): GB/s of SAM text and records/s
  kernel   text already in device memory (uploaded beforehand), the four kernels of one chunk only (dwgsim_hip_eval_debug_device_chunk)
  e2e      text in page-locked host memory fed through dwgsim_hip_eval_feed: copy into the context's slots, upload, kernels, results
  model    tests/eval_model.py, the plain-Python model, on one core
With --bam the same records are also measured as a BAM file (level 6, 64 KiB BGZF blocks, written by tests/bam_io.py):
  bam_kernel   the uncompressed records in device memory, k_eval_bam_records alone (dwgsim_hip_eval_debug_device_bam_chunk)
  bam_inflate  the BGZF blocks inflated on 1, 4, 8 and 16 host threads, no device involved (dwgsim_hip_eval_debug_inflate)
  bam_e2e      the BAM bytes fed through dwgsim_hip_eval_feed_bam at 1, 4, 8 and 16 inflate threads: GB/s of uncompressed BAM, records/s
With --breakdown every kernel and e2e figure is measured again in the same run with a breakdown set (dwgsim_hip_eval_set_breakdown): all four
dimensions at the default cap (keys bd_*, and bd_*_ratio = breakdown / plain time) and, for the kernels, at cap 32 (keys bd32_*).
--bam-threads LIST (default 1,4,8,16) chooses the inflate thread counts of bam_inflate and bam_e2e.
With --truth the records are measured once more under names of their own (every copy of the block renamed, so that no key is asked for
twice in a launch) against a truth SAM of --truth-copies sets of names (one record per name and end, one in eight with an insertion; the
asked records lie spread over the whole truth), in the same run on the same records:
  truth_load   header, feed and commit of that truth: records/s and GB/s of truth text (keys truth_*)
  dn_kernel    the plain form over that device-resident text (keys dn_*)
  tr_kernel    the truth form over it (keys tr_*, and tr_*_ratio = truth / plain time), SAM and, with --bam, BAM
Prints one JSON line.  Usage: python tools/eval_throughput.py [--mib 1024] [--reps 5] [--model-mib 16] [--a 3] [--bam] [--bam-threads 8] [--breakdown]
                                                              [--truth] [--truth-copies 100]"""
import argparse, ctypes as C, io, json, os, random, re, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from dwgsim_amd import api  # noqa: E402
import eval_model as M  # noqa: E402
import eval_sam as S  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--model-mib", type=int, default=16)
    ap.add_argument("--a", type=int, default=3)
    ap.add_argument("--bam", action="store_true")
    ap.add_argument("--breakdown", action="store_true")
    ap.add_argument("--bam-threads", default="1,4,8,16")
    ap.add_argument("--truth", action="store_true")
    ap.add_argument("--truth-copies", type=int, default=100)
    args = ap.parse_args()
    contigs = [("chr%d" % i, 200_000_000) for i in range(1, 23)]
    rng = random.Random(5)
    head = S.header(contigs)
    block = b"".join(r + b"\n" for r in S.records(rng, S.synth_names(rng, contigs, 40000), contigs))
    recs_block = block.count(b"\n")
    k = max(1, (args.mib << 20) // len(block))
    text = block * k
    n_bytes, n_recs = len(text), recs_block * k
    out = {"bytes": n_bytes, "records": n_recs, "a": args.a}

    lib = api.load()
    forms = FORMS if args.breakdown else FORMS[:1]
    for pre, kw in forms:
        with api.EvalContext(a=args.a, **kw) as ctx:
            ctx.header(head)
            ms = C.c_double()
            r = lib.dwgsim_hip_eval_debug_device_chunk(ctx.ctx, text, n_bytes, 1, C.byref(ms))      # warm-up
            r = r or lib.dwgsim_hip_eval_debug_device_chunk(ctx.ctx, text, n_bytes, args.reps, C.byref(ms))
            if r:
                raise SystemExit("device chunk failed: %d" % r)
            out[pre + "kernel_ms"] = ms.value
            out[pre + "kernel_GBps"] = n_bytes / ms.value / 1e6
            out[pre + "kernel_Mrec_s"] = n_recs / ms.value / 1e3
            if pre:
                out[pre + "kernel_ratio"] = ms.value / out["kernel_ms"]

    if args.truth:
        truth_throughput(lib, args, head, block, k, out)

    pinned = lib.dwgsim_hip_host_alloc(n_bytes)
    if not pinned:
        raise SystemExit("host_alloc failed")
    C.memmove(pinned, text, n_bytes)
    for pre, kw in forms[:2]:
        best = None
        for _ in range(args.reps):
            with api.EvalContext(a=args.a, **kw) as ctx:
                ctx.header(head)
                t0 = time.perf_counter()
                lib.dwgsim_hip_eval_feed(ctx.ctx, C.c_void_p(pinned), n_bytes)
                table, sm = ctx.finish()
                dt = time.perf_counter() - t0
            assert sm.status == 0 and sm.records == n_recs
            best = dt if best is None else min(best, dt)
        out[pre + "e2e_s"] = best
        out[pre + "e2e_GBps"] = n_bytes / best / 1e9
        out[pre + "e2e_Mrec_s"] = n_recs / best / 1e6
    lib.dwgsim_hip_host_free(C.c_void_p(pinned))

    if args.bam:
        bam_throughput(lib, args, head, block, k, out)

    sub = block * max(1, (args.model_mib << 20) // len(block))
    t0 = time.perf_counter()
    M.run([head + sub], M.Opts(a=args.a))
    dt = time.perf_counter() - t0
    out["model_GBps"] = len(sub) / dt / 1e9
    out["model_Mrec_s"] = sub.count(b"\n") / dt / 1e6
    print(json.dumps(out))


# key prefix and EvalContext arguments of the plain form, of the breakdown at the default cap, and of the breakdown at cap 32
FORMS = [("", {}), ("bd_", {"breakdown": "snps,errors,indels,end"}), ("bd32_", {"breakdown": "snps,errors,indels,end", "breakdown_cap": 32})]


def renamed(block, c):
    """the records of block under other names: copy c > 0 has #c behind every QNAME"""
    return block if c == 0 else re.sub(rb"(?m)^([^\t\n]+)\t", rb"\1#%d\t" % c, block)


def truth_for(head, block, copies):
    """a truth SAM over the records of block: every (QNAME, end) once, under the names of the copies 0 ... copies - 1 (renamed), the copies
    of one record next to each other, so that the records a run asks for lie spread over the whole truth"""
    seen, lines = set(), []
    for line in block.split(b"\n"):
        f = line.split(b"\t")
        if len(f) < 11:
            continue
        flag = int(f[1])
        end = (flag >> 6) & 3 if flag & 1 else 0
        if (f[0], end) in seen or (flag & 1 and end not in (1, 2)):
            continue
        seen.add((f[0], end))
        rname = f[2] if f[2] != b"*" else b"chr1"
        cigar = b"20M1I29M" if len(seen) % 8 == 0 else b"50M"
        lines.append((f[0], b"\t%d\t%s\t%d\t255\t%s\t*\t0\t0\tACGT\tIIII\n" % (flag & 0xD1, rname, max(1, int(f[3])), cigar)))
    suffix = [b""] + [b"#%d" % c for c in range(1, copies)]
    return head + b"".join(q + x + rest for q, rest in lines for x in suffix), len(lines) * copies


def truth_throughput(lib, args, head, block, k, out):
    """Every record of the measured text has a name of its own (the block's records under k sets of names), so every look-up of a launch
    goes to another slot and another record; the truth holds --truth-copies sets, the asked ones spread among them.  The plain form is
    measured on the same text in the same run (keys dn_*: distinct names)."""
    text = b"".join(renamed(block, c) for c in range(k))
    n_recs = text.count(b"\n")
    truth, n_truth = truth_for(head, block, max(args.truth_copies, k))
    out.update({"truth_records": n_truth, "truth_bytes": len(truth), "truth_records_asked_for": n_truth // max(args.truth_copies, k) * k,
                "dn_bytes": len(text), "dn_records": n_recs})
    best = None
    for _ in range(min(args.reps, 3)):
        with api.EvalContext(a=args.a) as ctx:
            t0 = time.perf_counter()
            ctx.load_truth(io.BytesIO(truth), 64 << 20)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
    out["truth_load_s"] = best
    out["truth_load_Mrec_s"] = n_truth / best / 1e6
    out["truth_load_GBps"] = len(truth) / best / 1e9
    times = {}
    for pre, with_truth in (("dn_", False), ("tr_", True)):
        with api.EvalContext(a=args.a) as ctx:
            if with_truth:
                ctx.load_truth(io.BytesIO(truth), 64 << 20)
            ctx.header(head)
            ms = C.c_double()
            r = lib.dwgsim_hip_eval_debug_device_chunk(ctx.ctx, text, len(text), 1, C.byref(ms))      # warm-up
            r = r or lib.dwgsim_hip_eval_debug_device_chunk(ctx.ctx, text, len(text), args.reps, C.byref(ms))
            if r:
                raise SystemExit("device chunk failed: %d" % r)
            times[pre] = ms.value
            out[pre + "kernel_ms"] = ms.value
            out[pre + "kernel_Mrec_s"] = n_recs / ms.value / 1e3
    out["tr_kernel_ratio"] = times["tr_"] / times["dn_"]
    if args.bam:
        import bam_io as B
        payload, offs = B.bam_payload(head + text)
        hdr, raw = payload[:offs[0]], payload[offs[0]:]
        for pre, with_truth in (("dn_", False), ("tr_", True)):
            with api.EvalContext(a=args.a) as ctx:
                if with_truth:
                    ctx.load_truth(io.BytesIO(truth), 64 << 20)
                ctx.bam_begin()
                ctx.feed_bam(B.bgzf(hdr, eof=False))
                ms = C.c_double()
                r = lib.dwgsim_hip_eval_debug_device_bam_chunk(ctx.ctx, raw, len(raw), 1, C.byref(ms))      # warm-up
                r = r or lib.dwgsim_hip_eval_debug_device_bam_chunk(ctx.ctx, raw, len(raw), args.reps, C.byref(ms))
                if r:
                    raise SystemExit("device BAM chunk failed: %d" % r)
                times[pre] = ms.value
                out[pre + "bam_kernel_ms"] = ms.value
        out["tr_bam_kernel_ratio"] = times["tr_"] / times["dn_"]


def bam_throughput(lib, args, head, block, k, out):
    import bam_io as B
    payload, offs = B.bam_payload(head + block)
    hdr, recs = payload[:offs[0]], payload[offs[0]:]
    n_recs = len(offs) * k
    # whole blocks of records only, so that the file is the header's blocks followed by k copies of the records' blocks
    rec_blocks = B.bgzf(recs, eof=False)
    bam = B.bgzf(hdr, eof=False) + rec_blocks * k + B.EOF_BLOCK
    raw = recs * k
    out.update({"bam_file_bytes": len(bam), "bam_record_bytes": len(raw), "bam_records": n_recs})

    forms = FORMS if args.breakdown else FORMS[:1]
    for pre, kw in forms:
        with api.EvalContext(a=args.a, **kw) as ctx:
            ctx.bam_begin()
            ctx.feed_bam(B.bgzf(hdr, eof=False))
            ms = C.c_double()
            r = lib.dwgsim_hip_eval_debug_device_bam_chunk(ctx.ctx, raw, len(raw), 1, C.byref(ms))      # warm-up
            r = r or lib.dwgsim_hip_eval_debug_device_bam_chunk(ctx.ctx, raw, len(raw), args.reps, C.byref(ms))
            if r:
                raise SystemExit("device BAM chunk failed: %d" % r)
            out[pre + "bam_kernel_ms"] = ms.value
            out[pre + "bam_kernel_GBps"] = len(raw) / ms.value / 1e6
            out[pre + "bam_kernel_Mrec_s"] = n_recs / ms.value / 1e3
            if pre:
                out[pre + "bam_kernel_ratio"] = ms.value / out["bam_kernel_ms"]

    pinned = lib.dwgsim_hip_host_alloc(len(bam))
    if not pinned:
        raise SystemExit("host_alloc failed")
    C.memmove(pinned, bam, len(bam))
    for t in [int(x) for x in args.bam_threads.split(",")]:
        ms, nb = C.c_double(), C.c_uint64()
        if lib.dwgsim_hip_eval_debug_inflate(C.c_void_p(pinned), len(bam), t, args.reps, C.byref(ms), C.byref(nb)):
            raise SystemExit("inflate failed")
        out["bam_inflate_GBps_t%d" % t] = nb.value / ms.value / 1e6
        for pre, kw in forms[:2]:
            best = None
            for _ in range(args.reps):
                with api.EvalContext(a=args.a, inflate_threads=t, **kw) as ctx:
                    ctx.bam_begin()
                    t0 = time.perf_counter()
                    step = 8 << 20
                    for i in range(0, len(bam), step):
                        lib.dwgsim_hip_eval_feed_bam(ctx.ctx, C.c_void_p(pinned + i), min(step, len(bam) - i))
                    table, sm = ctx.finish()
                    dt = time.perf_counter() - t0
                assert sm.status == 0 and sm.records == n_recs, (sm.status, sm.records, n_recs)
                best = dt if best is None else min(best, dt)
            out[pre + "bam_e2e_GBps_t%d" % t] = (len(raw) + len(hdr)) / best / 1e9
            out[pre + "bam_e2e_Mrec_s_t%d" % t] = n_recs / best / 1e6
    lib.dwgsim_hip_host_free(C.c_void_p(pinned))


if __name__ == "__main__":
    main()
