"""Throughput of the haplotype FASTA (dwgsim_hip_haplotype_fasta; DESIGN.md "6d"; not part of bench.py), on one device.
For the chr20-sized contig of bench.py's workload and for the 5000 scaffolds of `assembly5k` as ONE group, haplotype 1 at --width:
  len_us     the length pass and the scan of its block counts (HIP events; dwgsim_hip_debug_get "hap_len_us")
  write_us   the header and write kernels ("hap_write_us"); write_GBps = text bytes / write_us
  copy_us    a device-to-device hipMemcpyAsync of the same byte count, behind the text on the same stream in the same call ("hap_yardstick" /
             "hap_copy_us"): the yardstick; copy_GBps, and ratio = write_GBps / copy_GBps
  call_ms    the whole call on the host clock: both passes, the prefix read back, the records placed and uploaded, the waits
Each is the best of --reps builds (the text is built again by asking for another width in between).  fetch_GBps: the text copied to
page-locked host memory in one dwgsim_hip_haplotype_fetch.
With --cli: dwgsim-hip on the chr20-sized FASTA (bench.py's flags at --cli-cov) with and without DWGSIM_HIP_HAPLOTYPES, --cli-reps alternating runs
each, wall seconds.  Prints one JSON line.
Usage: python tools/hapfasta_throughput.py [--reps 5] [--width 60] [--workloads chr20,assembly5k] [--cli] [--cli-cov 30] [--cli-reps 3]"""
import argparse, ctypes as C, json, os, subprocess, sys, tempfile, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dwgsim_amd import api, synth  # noqa: E402

FLAGS = "-z 13 -1 150 -2 150 -C 30 -o 1"      # bench.py's


def measure(lib, contigs, width, reps):
    out = {"contigs": len(contigs), "bases": int(sum(len(a) for _, a in contigs))}
    with api.Context(api.parse_flags(FLAGS, lib), 0, lib) as ctx:
        h0 = ctx.add_contigs(contigs)
        ctx.mutate(h0)
        ctx.debug_option("hap_yardstick", 1)
        n = C.c_uint64(0)
        best = {}
        for r in range(reps + 1):      # (the first build allocates: not counted)
            ctx._chk(lib.dwgsim_hip_haplotype_fasta(ctx.h, h0, 0, width + 1, C.byref(n)))
            t0 = time.perf_counter()
            ctx._chk(lib.dwgsim_hip_haplotype_fasta(ctx.h, h0, 0, width, C.byref(n)))
            call_ms = 1e3 * (time.perf_counter() - t0)
            if r:
                for k, v in (("len_us", ctx.debug_get("hap_len_us")), ("write_us", ctx.debug_get("hap_write_us")), ("copy_us", ctx.debug_get("hap_copy_us")), ("call_ms", call_ms)):
                    best[k] = v if k not in best else min(best[k], v)
        out.update(best)
        out["text_bytes"] = n.value
        out["write_GBps"] = n.value / max(best["write_us"], 1) / 1e3
        out["copy_GBps"] = n.value / max(best["copy_us"], 1) / 1e3
        out["ratio"] = out["write_GBps"] / out["copy_GBps"]
        p = lib.dwgsim_hip_host_alloc(n.value)
        if p:
            dt = None
            for _ in range(3):
                t0 = time.perf_counter()
                ctx._chk(lib.dwgsim_hip_haplotype_fetch(ctx.h, 0, 0, p, n.value))
                d = time.perf_counter() - t0
                dt = d if dt is None else min(dt, d)
            out["fetch_GBps"] = n.value / dt / 1e9
            lib.dwgsim_hip_host_free(p)
        ctx.drop_contig(h0)
    return out


def cli_runs(contigs, cov, reps):
    cli = os.path.join(ROOT, "dwgsim_amd", "dwgsim-hip")
    flags = FLAGS.replace("-C 30", f"-C {cov}")
    out = {"flags": flags, "plain_s": [], "haplotypes_s": []}
    with tempfile.TemporaryDirectory() as t:
        fa = os.path.join(t, "ref.fa")
        synth.write_fasta(fa, contigs)
        base = {k: v for k, v in os.environ.items() if not k.startswith("DWGSIM_HIP_HAPLOTYPES")}
        for r in range(reps):
            for key, env in (("plain_s", base), ("haplotypes_s", dict(base, DWGSIM_HIP_HAPLOTYPES="1"))):
                t0 = time.perf_counter()
                subprocess.run([cli] + flags.split() + [fa, os.path.join(t, key)], check=True, stderr=subprocess.DEVNULL, env=env)
                out[key].append(round(time.perf_counter() - t0, 3))
        out["hap_file_bytes"] = os.path.getsize(os.path.join(t, "haplotypes_s.hap1.fa")) + os.path.getsize(os.path.join(t, "haplotypes_s.hap2.fa"))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--width", type=int, default=60)
    ap.add_argument("--workloads", default="chr20,assembly5k")
    ap.add_argument("--cli", action="store_true")
    ap.add_argument("--cli-cov", type=float, default=30)
    ap.add_argument("--cli-reps", type=int, default=3)
    args = ap.parse_args()
    lib = api.load()
    if lib.dwgsim_hip_device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")
    out = {"width": args.width, "reps": args.reps}
    for w in [x for x in args.workloads.split(",") if x]:
        contigs = synth.workload_contigs(w)
        out[w] = measure(lib, contigs, args.width, args.reps)
        if args.cli and w == "chr20":
            out["cli_chr20"] = cli_runs(contigs, args.cli_cov, args.cli_reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
