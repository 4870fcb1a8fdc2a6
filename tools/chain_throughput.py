"""Throughput of the chain step (dwgsim_hip_haplotype_chain; DESIGN.md "6g"; not part of bench.py), on one device.
For the chr20-sized contig of bench.py's workload and for the 5000 scaffolds of `assembly5k` as ONE group, per haplotype:
  count_us   the count pass and the scan of its block counts (HIP events; dwgsim_hip_debug_get "chain_count_us")
  write_us   the write pass ("chain_write_us"); device_us = count_us + write_us
  blocks     the ungapped blocks of the group ("chain_blocks")
  call_ms    the whole call on the host clock: both passes, the prefix and the entries read back, the pairing, the waits
  host_ms    the blocks of every contig fetched (dwgsim_hip_chain_blocks) and formatted in both directions (dwgsim_hip_chain_format); text_bytes of one direction
and, in the same process on the same group, the yardstick: len_us, the haplotype FASTA's length pass + scan ("hap_len_us"), which also reads every cell
once; ratio = device_us / len_us.  Each time is the best of --reps builds (the group is walked again in between: that is what makes a chain go).
With --cli: dwgsim-hip on the chr20-sized FASTA (bench.py's flags at --cli-cov) with and without DWGSIM_HIP_CHAIN, --cli-reps alternating runs each, wall
seconds.  Prints one JSON line.
Usage: python tools/chain_throughput.py [--reps 5] [--workloads chr20,assembly5k] [--cli] [--cli-cov 30] [--cli-reps 3]"""
import argparse, ctypes as C, json, os, subprocess, sys, tempfile, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dwgsim_amd import api, synth  # noqa: E402

FLAGS = "-z 13 -1 150 -2 150 -C 30 -o 1"      # bench.py's


def host_part(ctx, lib, h0, contigs, hap):
    """every contig's blocks fetched and formatted, both directions: (seconds, bytes of one direction)"""
    t0 = time.perf_counter()
    size, cid = 0, 1
    n, r0 = C.c_uint64(0), C.c_int64(0)
    for k, (name, arr) in enumerate(contigs):
        ctx._chk(lib.dwgsim_hip_chain_blocks(ctx.h, h0 + k, hap, C.byref(n), C.byref(r0), None, 0))
        if n.value == 0:
            continue
        blk = (api.ChainBlock * n.value)()
        ctx._chk(lib.dwgsim_hip_chain_blocks(ctx.h, h0 + k, hap, None, None, blk, n.value))
        for d in (api.CHAIN_TO_REF, api.CHAIN_FROM_REF):
            need = lib.dwgsim_hip_chain_format(name.encode(), len(arr), r0.value, blk, n.value, d, cid, None, 0)
            buf = C.create_string_buffer(need + 1)
            lib.dwgsim_hip_chain_format(name.encode(), len(arr), r0.value, blk, n.value, d, cid, buf, need)
        size += need
        cid += 1
    return time.perf_counter() - t0, size


def measure(lib, contigs, reps):
    out = {"contigs": len(contigs), "bases": int(sum(len(a) for _, a in contigs))}
    with api.Context(api.parse_flags(FLAGS, lib), 0, lib) as ctx:
        h0 = ctx.add_contigs(contigs)
        n = C.c_uint64(0)
        for hap in (0, 1):
            best = {}
            for r in range(reps + 1):      # (the first build allocates: not counted)
                ctx.mutate(h0)
                ctx._chk(lib.dwgsim_hip_haplotype_fasta(ctx.h, h0, hap, 60, None))
                len_us = ctx.debug_get("hap_len_us")
                t0 = time.perf_counter()
                ctx._chk(lib.dwgsim_hip_haplotype_chain(ctx.h, h0, hap, C.byref(n)))
                call_ms = 1e3 * (time.perf_counter() - t0)
                host_s, size = host_part(ctx, lib, h0, contigs, hap)
                cu, wu = ctx.debug_get("chain_count_us"), ctx.debug_get("chain_write_us")
                if r:
                    for k, v in (("count_us", cu), ("write_us", wu), ("device_us", cu + wu), ("len_us", len_us), ("call_ms", call_ms), ("host_ms", 1e3 * host_s)):
                        best[k] = v if k not in best else min(best[k], v)
            best.update(blocks=ctx.debug_get("chain_blocks"), text_bytes=size, ratio=best["device_us"] / max(best["len_us"], 1), count_ratio=best["count_us"] / max(best["len_us"], 1))
            assert best["blocks"] == n.value
            out[f"hap{hap + 1}"] = best
        ctx.drop_contig(h0)
    return out


def cli_runs(contigs, cov, reps):
    cli = os.path.join(ROOT, "dwgsim_amd", "dwgsim-hip")
    flags = FLAGS.replace("-C 30", f"-C {cov}")
    out = {"flags": flags, "plain_s": [], "chain_s": []}
    with tempfile.TemporaryDirectory() as t:
        fa = os.path.join(t, "ref.fa")
        synth.write_fasta(fa, contigs)
        base = {k: v for k, v in os.environ.items() if k != "DWGSIM_HIP_CHAIN" and not k.startswith("DWGSIM_HIP_HAPLOTYPES")}
        for r in range(reps):
            for key, env in (("plain_s", base), ("chain_s", dict(base, DWGSIM_HIP_CHAIN="1"))):
                t0 = time.perf_counter()
                subprocess.run([cli] + flags.split() + [fa, os.path.join(t, key)], check=True, stderr=subprocess.DEVNULL, env=env)
                out[key].append(round(time.perf_counter() - t0, 3))
        out["chain_file_bytes"] = sum(os.path.getsize(os.path.join(t, f"chain_s.hap{h}.{d}.chain")) for h in (1, 2) for d in ("to_ref", "from_ref"))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--workloads", default="chr20,assembly5k")
    ap.add_argument("--cli", action="store_true")
    ap.add_argument("--cli-cov", type=float, default=30)
    ap.add_argument("--cli-reps", type=int, default=3)
    args = ap.parse_args()
    lib = api.load()
    if lib.dwgsim_hip_device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")
    out = {"reps": args.reps}
    for w in [x for x in args.workloads.split(",") if x]:
        contigs = synth.workload_contigs(w)
        out[w] = measure(lib, contigs, args.reps)
        if args.cli and w == "chr20":
            out["cli_chr20"] = cli_runs(contigs, args.cli_cov, args.cli_reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
