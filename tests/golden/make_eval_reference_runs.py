#!/usr/bin/env python3
"""Record what the UNMODIFIED reference evaluator (oracle/_ref/dwgsim_eval: the reference's dwgsim_eval.c, compiled where it lies and linked
with oracle/samshim by `make -C oracle ref`) answers on the cases of tests/eval_reference_cases.py, into
tests/golden/eval_reference_runs.json, so that tests/test_eval_reference.py and tests/test_gpu_eval_reference.py run without the reference.

  inputs   name -> sha256 of every input file (made again from seeds by the case list, or a fixture under tests/golden/eval/)
  runs     case id -> args (options, then the input names), files, rc, stderr (after the one normalisation rule of
           eval_reference_cases.normalize_stderr), and unless the run ended on a fatal record: sha256 and length of stdout, and stdout itself
           when it is at most 4 KiB (wide tables are hashes, to keep this file small).  With -p, stdout is taken from the line `# thr |` on.
  single   the single-record runs on awkward names: the fixture's sha256, the option sets, the distinct answers (as in `runs`) and, per option
           set, the index of the answer to record k of the fixture.  The input of run k is eval_reference_cases.single_input(k).

usage: python tests/golden/make_eval_reference_runs.py            writes tests/golden/eval/awkward.sam and eval_reference_runs.json
       python tests/golden/make_eval_reference_runs.py --check    runs the reference again and compares with the committed files
       ... --check --san    the same through oracle/_ref/dwgsim_eval_san (`make -C oracle ref-san`: the shim under ASan and UBSan)"""
import json, os, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import eval_reference_cases as R


def answer(binary, args, paths, cwd, p_on):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")          # (the reference leaves through exit() on a fatal record and frees nothing)
    p = subprocess.run([binary] + args + paths, capture_output=True, cwd=cwd, timeout=600, env=env)
    a = {"rc": p.returncode, "stderr": R.normalize_stderr(p.stderr).decode("latin-1")}
    if p.returncode == 0:
        out = R.table_part(p.stdout) if p_on else p.stdout
        a["stdout_sha256"] = R.sha256(out); a["stdout_len"] = len(out)
        if len(out) <= R.STORE_STDOUT:
            a["stdout"] = out.decode("latin-1")
    return a


def make(binary=R.REF_EVAL):
    """the whole record, from the reference at `binary`"""
    ins, cases = R.inputs(), R.cases()
    head, lines = R.awkward()
    rec = {"reference": "nh13/DWGSIM v0.1.17-dev src/dwgsim_eval.c, compiled unmodified and linked with oracle/samshim (oracle/Makefile)",
           "inputs": {name: R.sha256(data) for name, data in sorted(ins.items())}, "runs": {}, "single": {}}
    with tempfile.TemporaryDirectory() as t, ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        for name, data in ins.items():
            with open(os.path.join(t, name), "wb") as f:
                f.write(data)

        def one(cid):
            c = cases[cid]
            args = R.argv(c["opts"], not R.is_bam(c["files"][0]))
            a = answer(binary, args, c["files"], t, c["opts"].get("p"))
            return cid, dict({"args": args + c["files"], "files": c["files"]}, **a)
        rec["runs"] = dict(ex.map(one, sorted(cases)))

        for k in range(len(lines)):
            with open(os.path.join(t, "awk%d" % k), "wb") as f:
                f.write(R.single_input(k))

        def single(job):
            name, k = job
            return answer(binary, R.argv(R.SINGLE_OPTS[name], True), ["awk%d" % k], t, False)
        jobs = [(name, k) for name in R.SINGLE_OPTS for k in range(len(lines))]
        answers, seen, index = [], {}, {name: [] for name in R.SINGLE_OPTS}
        for (name, k), a in zip(jobs, ex.map(single, jobs)):
            key = json.dumps(a, sort_keys=True)
            if key not in seen:
                seen[key] = len(answers); answers.append(a)
            index[name].append(seen[key])
    rec["single"] = {"fixture": "eval/awkward.sam", "sha256": R.sha256(R.join(head, lines)), "records": len(lines),
                     "options": {name: R.argv(o, True) for name, o in R.SINGLE_OPTS.items()}, "answers": answers, "index": index}
    return rec


def differences(old, new):
    out = []
    for sec in ("inputs", "runs"):
        for k in sorted(set(old[sec]) | set(new[sec])):
            if old[sec].get(k) != new[sec].get(k):
                out.append("%s[%s]" % (sec, k))
    so, sn = old["single"], new["single"]
    for k in ("sha256", "records", "options"):
        if so.get(k) != sn.get(k):
            out.append("single." + k)
    for name in set(so["index"]) | set(sn["index"]):
        a = [so["answers"][i] for i in so["index"].get(name, [])]; b = [sn["answers"][i] for i in sn["index"].get(name, [])]
        out += ["single/%s/%d" % (name, k) for k in range(max(len(a), len(b))) if a[k:k + 1] != b[k:k + 1]]
    return out


def main():
    check = "--check" in sys.argv[1:]
    binary = R.REF_EVAL + "_san" if "--san" in sys.argv[1:] else R.REF_EVAL
    if not os.path.exists(binary):
        raise SystemExit(f"{binary} is missing: build it with `make -C oracle ref` where the reference sources are present")
    text = R.awkward_sam()
    if check:
        with open(R.AWKWARD, "rb") as f:
            if f.read() != text:
                raise SystemExit("tests/golden/eval/awkward.sam is not what eval_reference_cases.awkward_sam() writes: record again")
        diff = differences(R.record(), make(binary))
        if diff:
            raise SystemExit("the reference no longer answers as recorded (%d differences): %s" % (len(diff), ", ".join(diff[:20])))
        print("eval_reference_runs.json: the reference answers as recorded")
        return
    with open(R.AWKWARD, "wb") as f:
        f.write(text)
    R.awkward.cache_clear()
    rec = make(binary)
    with open(R.RECORD, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    s = rec["single"]
    print(f"eval_reference_runs.json: {len(rec['runs'])} runs, {s['records']} x {len(s['options'])} single-record runs "
          f"({len(s['answers'])} distinct answers), {os.path.getsize(R.RECORD)} bytes")


if __name__ == "__main__":
    main()
