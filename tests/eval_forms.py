"""What the record loop of dwgsim_eval-hip promises whatever the form of the record kernel (dw_eval.hip: Plain, Breakdown, Truth) and whatever
the front (SAM, BAM): the main table, n, records, the -p text, stderr, and the first fatal record.  One file, 4096-byte chunks, -m 1 -p 1 -a 3,
so that records, -m pairs, the context record and the spill list all cross many chunk boundaries.  test_eval_forms_emu.py runs it on the CPU
emulation and test_gpu_eval_forms.py on the device; the plain-Python model (eval_model.py) is the reference."""
import ctypes as C, io, random
from types import SimpleNamespace

import bam_io as B
import eval_model as M
import eval_sam as S
from dwgsim_amd import api

CONTIGS = [("chr1", 5000), ("chr10", 3000), ("chr2_alt", 2000)]
OPTS = {"m": 1, "p": 1, "a": 3}
CHUNK = 4096
FRONTS = ["sam", "bam"]
CODES = [M.E_MALFORMED, M.E_NAME, M.E_CONTIG, M.E_PAIRED]
WHERE = 0.37


def sam_file() -> bytes:
    """300 pairs, about 640 records, with scores far outside the kernel's window"""
    return S.sam_file(random.Random(31), CONTIGS, 300, wide_scores=True)


def forms(sam: bytes) -> dict:
    """the arguments that choose each form; the truth holds only the header, so every mapped record is `missing` and the truth form runs"""
    return {"plain": {}, "breakdown": {"breakdown": "snps,errors,indels,end"}, "truth": {"truth": M.split_header(sam)[0]}}


def text_of(ctx, call) -> bytes:
    txt, ln = C.c_void_p(), C.c_size_t()
    assert call(ctx.ctx, C.byref(txt), C.byref(ln)) == 0
    return C.string_at(txt, ln.value) if ln.value else b""


def run(lib, front: str, data: bytes, form: dict, **o):
    """(table, summary) of one file through one front in one form, fed in pieces of 1000 bytes.  Of the breakdown's and the truth's text the
    summary has only the lengths: with scores this wide the sections of a breakdown are tens of megabytes, which nothing here reads."""
    kw = dict(form)
    truth = kw.pop("truth", None)
    with api.EvalContext(lib=lib, chunk_bytes=CHUNK, **kw, **o) as ctx:
        if truth is not None:
            ctx.load_truth(io.BytesIO(truth))
        if front == "bam":
            ctx.bam_begin()
            feed = ctx.feed_bam
        else:
            head, data = M.split_header(data)
            ctx.header(head)
            feed = ctx.feed
        for i in range(0, len(data), 1000):
            if not feed(data[i:i + 1000]):
                break
        sm = api.EvalSummary()
        sm.size = C.sizeof(api.EvalSummary)
        assert lib.dwgsim_hip_eval_finish(ctx.ctx, C.byref(sm)) == 0
        res = SimpleNamespace(status=sm.status, error_code=sm.error_code, error_record=sm.error_record, n=sm.n, records=sm.records,
                              stderr=C.string_at(sm.stderr_text, sm.stderr_len), incorrect=text_of(ctx, lib.dwgsim_hip_eval_incorrect_text),
                              breakdown_bytes=len(text_of(ctx, lib.dwgsim_hip_eval_breakdown_text)),
                              truth_bytes=len(text_of(ctx, lib.dwgsim_hip_eval_truth_text)))
        return text_of(ctx, lib.dwgsim_hip_eval_table_text), res


def inputs(sam: bytes) -> dict:
    """front -> (what the run reads, the SAM text that the model reads: a BAM run prints the -p records as it decodes them)"""
    bam = B.sam_to_bam(sam, block_bytes=700)
    return {"sam": (sam, sam), "bam": (bam, B.bam_to_sam(bam))}


def check_forms_agree(lib, front: str, sam: bytes):
    data, text = inputs(sam)[front]
    want = M.run([text], M.Opts(**OPTS))
    assert want.status == 0 and want.incorrect.count(b"\n") > 50 and want.table.count(b"\n") > 300
    for name, form in forms(sam).items():
        table, sm = run(lib, front, data, form, **OPTS)
        got = (sm.status, table, sm.n, sm.records, sm.incorrect, sm.stderr)
        assert got == (0, want.table, want.n, len(M.record_lines(M.split_header(text)[1])), want.incorrect, want.stderr), name
        assert bool(sm.breakdown_bytes) == (name == "breakdown") and bool(sm.truth_bytes) == (name == "truth")


BAD_LINE = {
    M.E_MALFORMED: b"three\tfields\tonly",
    M.E_NAME: b"not_from_dwgsim\t65\tchr1\t100\t60\t50M\t=\t0\t0\tA\tI",
    M.E_CONTIG: b"nochr_100_200_0_0_0_0_0:0:0_0:0:0_1\t65\t*\t0\t0\t*\t*\t0\t0\tA\tI",
}


def fatal_case(sam: bytes, code: int, front: str):
    """(what the run reads, the text the model reads, the options, the damaged record's number): record int(WHERE * records) of the file
    replaced by one with that fatal code.  A record that BAM cannot hold (too few fields) is made in the BAM file itself: a read name of no
    bytes.  E_PAIRED exists only under -z, where the first paired record of a file is fatal: there the records in front of the damaged one
    lose their pairing bits, which makes it the first paired one."""
    head, body = M.split_header(sam)
    lines = M.record_lines(body)
    k = int(WHERE * len(lines))
    o = dict(OPTS)
    if code == M.E_PAIRED:
        o["z"] = 1
        for i in range(k):
            f = lines[i].split(b"\t")
            f[1] = b"%d" % (int(f[1]) & ~0xC1)
            lines[i] = b"\t".join(f)
    else:
        lines[k] = BAD_LINE[code]
    text = head + b"".join(l + b"\n" for l in lines)
    if front == "sam":
        return text, text, o, k
    if code == M.E_MALFORMED:
        lines[k] = BAD_LINE[M.E_NAME]           # (a record of any kind to encode; the patch makes it malformed)
        payload, offs = B.bam_payload(head + b"".join(l + b"\n" for l in lines))
        p = bytearray(payload)
        p[offs[k] + 12] = 1                     # l_read_name: the NUL alone
        return B.bgzf(bytes(p), 700), text, o, k
    bam = B.sam_to_bam(text, block_bytes=700)
    return bam, B.bam_to_sam(bam), o, k


def check_fatal_record(lib, front: str, sam: bytes, code: int):
    data, text, o, k = fatal_case(sam, code, front)
    want = M.run([text], M.Opts(**o))
    assert (want.status, want.error_code, want.error_record) == (1, code, k)
    for name, form in forms(sam).items():
        table, sm = run(lib, front, data, form, **o)
        assert (sm.status, sm.error_code, sm.error_record, sm.stderr, table) == (1, code, k, want.stderr, b""), name
