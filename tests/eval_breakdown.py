"""Test-only helper for the breakdown tests of dwgsim_eval-hip (test_eval_breakdown_emu.py on the CPU emulation, test_gpu_eval_breakdown.py on
the GPU): what every section of a breakdown must be, made from the plain-Python model (eval_model.py) alone -- its filter runs (-s k, -e k,
-i) and its table formatter.  Nothing here reads product code."""
from __future__ import annotations
import eval_model as M
import eval_sam as S

ALL = "snps,errors,indels,end"


def opts(o: dict, **more) -> M.Opts:
    d = dict(o); d.update(more)
    return M.Opts(**{k: (v.encode() if k == "P" and isinstance(v, str) else v) for k, v in d.items()})


def add(*hists) -> dict:
    out: dict = {}
    for h in hists:
        for sc, row in h.items():
            acc = out.setdefault(sc, [0] * 5)
            for c in range(5):
                acc[c] += row[c]
    return out


def sub(a: dict, b: dict) -> dict:
    out = {sc: list(row) for sc, row in a.items()}
    for sc, row in b.items():
        for c in range(5):
            out[sc][c] -= row[c]
    assert all(v >= 0 for row in out.values() for v in row)
    return {sc: row for sc, row in out.items() if any(row)}


def parse_table(table: bytes) -> dict:
    """the per-score counts of a table text (the test's own reading of the rows: thr mc mi mu um uu ...), for a d of 1"""
    hist = {}
    for line in table.splitlines():
        if line.startswith(b"#") or not line:
            continue
        f = line.split()
        row = [int(x) for x in f[1:6]]
        if any(row):
            hist[int(f[0])] = row
    return hist


def by_end(files):
    """the files' records split by FLAG 0x40: ([(header, first-end lines)], [(header, the others)])"""
    first, second = [], []
    for data in files:
        head, body = M.split_header(data)
        lines = M.record_lines(body)
        first.append((head, [l for l in lines if int(l.split(b"\t")[1]) & 0x40]))
        second.append((head, [l for l in lines if not int(l.split(b"\t")[1]) & 0x40]))
    return first, second


def expected(files, o: dict, dims: str, cap: int, max_count: int, end: bool = True) -> dict:
    """label -> table text.  o holds none of i, e, s (the strata are compared with those filter runs); max_count: no name of the files
    holds a larger n_err_1 or n_sub_1, and none a negative one.  end=False leaves the end sections out (runs with -m)."""
    assert not ({"i", "e", "s"} & set(o))
    key = (tuple(files), tuple(sorted(o.items())), dims, cap, max_count, end)
    if key not in _EXPECTED:
        _EXPECTED[key] = _expected(files, o, dims, cap, max_count, end)
    return _EXPECTED[key]


_EXPECTED: dict = {}      # computed once per input and option set, shared by the tests that need it (read only)


def _expected(files, o, dims, cap, max_count, end):
    a, d = o.get("a", 0), o.get("d", 1)
    out = {}
    for dim, flt in (("snps", "s"), ("errors", "e")):
        if dim in dims.split(","):
            for k in range(cap):
                out["%s=%d" % (dim, k)] = M.run(files, opts(o, **{flt: k})).table
            rest = add(*[M.run(files, opts(o, **{flt: k})).hist for k in range(cap, max_count + 1)])
            out["%s=%d+" % (dim, cap)] = M.format_table(rest, a, d)
    if "indels" in dims.split(","):
        whole, with_indels = M.run(files, opts(o)), M.run(files, opts(o, i=1))
        out["indels=0"] = M.format_table(sub(whole.hist, with_indels.hist), a, d)
        out["indels=1+"] = with_indels.table
    if "end" in dims.split(",") and end:
        if o.get("z"):
            out["end=1"] = M.run(files, opts(o)).table
            out["end=2"] = M.format_table({}, a, d)
        else:
            first, second = by_end(files)
            out["end=1"] = M.run(first, opts(o)).table
            out["end=2"] = M.run(second, opts(o)).table
    return out


def labels(dims: str, cap: int):
    """the section labels in the order of the text"""
    out = []
    for dim in ("snps", "errors", "indels", "end"):
        if dim in dims.split(","):
            if dim in ("snps", "errors"):
                out += ["%s=%d" % (dim, k) for k in range(cap)] + ["%s=%d+" % (dim, cap)]
            else:
                out += [dim + "=" + s for s in (("0", "1+") if dim == "indels" else ("1", "2"))]
    return out


def check_sections(got: dict, want: dict, dims: str, cap: int, end: bool = True):
    assert list(got) == labels(dims, cap)
    for label, table in want.items():
        assert got[label] == table, label
    assert set(want) == set(l for l in got if end or not l.startswith("end="))


def check_partition(got: dict, table: bytes, dims: str, cap: int):
    """the strata of every dimension add up to the main table (d = 1)"""
    main = parse_table(table)
    for dim in dims.split(","):
        parts = [parse_table(t) for label, t in got.items() if label.startswith(dim + "=")]
        assert parts and add(*parts) == main, dim


def sparse_chunk(sam: bytes, blank: int = 400):
    """(header, text): every record line of `sam` followed by `blank` empty lines.  An empty line is a record of its own that counts nowhere, so
    a block of the breakdown kernel (512 lanes, one block per 128 KiB of text) makes len(lines) / (blocks * 512) turns of its record loop:
    more than the 127 after which it merges its 16-bit counters.  turns: that number for the text."""
    head, body = M.split_header(sam)
    text = b"".join(l + b"\n" * (1 + blank) for l in M.record_lines(body))
    blocks = ((len(text) + 65535) // 65536 + 1) // 2
    return head, text, text.count(b"\n") // (blocks * 512)


def many_count_names(contigs, n=410, top=40):
    """dwgsim names whose n_err_1 and n_sub_1 run over 0 ... top (each value several times, in different combinations)"""
    names = []
    for k in range(n):
        c, l = contigs[k % len(contigs)]
        p1 = 1 + (k * 37) % max(2, l - 400)
        names.append(S.dwgsim_name(c, p1, p1 + k % 200, k & 1, (k >> 1) & 1, int(k % 11 == 0), int(k % 11 == 0), k % (top + 1), (k * 7) % (top + 1),
                                   k % 2, (k * 3) % (top + 1), (k * 5) % (top + 1), (k // 2) % 2, k))
    return names
