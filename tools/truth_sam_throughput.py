"""Cost of the truth step (dwgsim_hip_set_truth_sam; DESIGN.md "6e"; not part of bench.py), on one device.
One batch of --pairs pairs (default 2^18) of the chr20-sized contig of bench.py's workload at 2 x 150, bench.py's flags:
  truth_us      the truth step's kernels -- record index, length passes, scan, write pass -- between two HIP events (dwgsim_hip_debug_get "truth_us")
  simulate_us   the same batch's k_simulate (dwgsim_hip_batch_t.sim_kernel_ms)
  copy_us       a device-to-device copy of the SAM's bytes on the same stream (dwgsim_hip_debug_option "truth_yardstick" / "truth_copy_us"): the yardstick;
                truth_GBps / copy_GBps = bytes over the two times
  plain_*       the same batch with the feature off: its k_simulate and kernel times (nothing of the step runs)
--md: the same with dwgsim_hip_set_truth_md on top (NM:i: and MD:Z: on every mapped record); the line then also holds "md": true and "truth_reruns" (second
runs for want of room: 0 on this workload).
--depth: the counters of the true read depth (dwgsim_hip_set_truth_depth; DESIGN.md "6f") on top.  The line then also holds "depth": three rounds that alternate the
truth step without the counters ("truth_us") and with them ("truth_depth_us": k_truth_depth behind k_truth_len, between the same two events), then the counters
without the truth SAM ("depth_alone_us": k_truth_len<false, false> and k_truth_depth, nothing else), the listed cells and the sum of all counters.
Each is the best of --reps batches (the first one allocates: not counted).  Prints one JSON line.
Usage: python tools/truth_sam_throughput.py [--reps 5] [--pairs 262144] [--md] [--depth]"""
import argparse, json, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dwgsim_amd import api, synth  # noqa: E402

FLAGS = "-z 13 -1 150 -2 150 -C 30 -o 1"      # bench.py's


def batches(ctx, h, pairs, reps, timed=False):
    best = {}
    last = None
    for r in range(reps + 1):
        b = ctx.simulate(h, r * pairs, pairs, 0, 0)
        if r:
            for k, v in (("simulate_us", 1e3 * b.sim_kernel_ms), ("kernels_us", 1e3 * b.kernel_ms), ("truth_us", ctx.debug_get("truth_us") if b.sam_bytes or timed else 0)):
                best[k] = v if k not in best else min(best[k], v)
        last = b
    return best, last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=1 << 18)
    ap.add_argument("--md", action="store_true", help="with NM:i: and MD:Z: (dwgsim_hip_set_truth_md)")
    ap.add_argument("--depth", action="store_true", help="also: the truth step with and without the counters of the true read depth, and the counters alone (dwgsim_hip_set_truth_depth)")
    args = ap.parse_args()
    lib = api.load()
    if lib.dwgsim_hip_device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")
    out = {"flags": FLAGS, "pairs": args.pairs, "reps": args.reps, "md": bool(args.md)}
    contigs = synth.workload_contigs("chr20")
    with api.Context(api.parse_flags(FLAGS, lib), 0, lib) as ctx:
        h = ctx.add_contigs(contigs)
        ctx.mutate(h)
        plain, _ = batches(ctx, h, args.pairs, args.reps)
        out.update({"plain_simulate_us": plain["simulate_us"], "plain_kernels_us": plain["kernels_us"]})
        ctx.set_truth_sam(True)
        if args.md:
            ctx.set_truth_md(True)
        on, b = batches(ctx, h, args.pairs, args.reps)
        out.update(on)
        out["sam_bytes"] = int(b.sam_bytes); out["fastq_bytes"] = int(b.bytes[0] + b.bytes[1])
        best = None
        for _ in range(args.reps + 1):
            ctx.debug_option("truth_yardstick", int(b.sam_bytes))
            us = ctx.debug_get("truth_copy_us")
            best = us if best is None else min(best, us)
        out["copy_us"] = best
        out["truth_GBps"] = b.sam_bytes / max(on["truth_us"], 1) / 1e3
        out["copy_GBps"] = b.sam_bytes / max(best, 1) / 1e3
        out["truth_over_simulate"] = on["truth_us"] / max(on["simulate_us"], 1)
        if args.md:
            out["truth_reruns"] = ctx.debug_get("truth_reruns")
        if args.depth:
            rounds = []
            for _ in range(3):
                ctx.set_truth_depth(False)
                off, _b = batches(ctx, h, args.pairs, args.reps)
                ctx.set_truth_depth(True)
                with_d, _b = batches(ctx, h, args.pairs, args.reps)
                rounds.append({"truth_us": off["truth_us"], "truth_depth_us": with_d["truth_us"], "simulate_us": with_d["simulate_us"]})
            ctx.set_truth_sam(False)
            alone, b = batches(ctx, h, args.pairs, args.reps, timed=True)
            counts = ctx.truth_depth(h)
            out["depth"] = {"rounds": rounds, "depth_alone_us": alone["truth_us"], "alone_simulate_us": alone["simulate_us"], "alone_sam_bytes": int(b.sam_bytes),
                            "listed_cells": int(len(counts)), "counter_sum": int(counts.sum())}
        ctx.drop_contig(h)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
