#!/usr/bin/env python3
"""tests/emu/check_lds.py LIB SOURCE... -- TEST INFRASTRUCTURE ONLY: after the link of an emulation library, check that the range lds.ld makes
(hipemu_lds_begin .. hipemu_lds_end, poisoned at every block start under HIPEMU_WAVES_APART) holds every __shared__ object the SOURCES declare, and
nothing else.  In the emulation a __shared__ object is a static local of its dw:: function; nm names it dw::<function>::<variable>."""
import re, subprocess, sys

lib, sources = sys.argv[1], sys.argv[2:]
names = set()
for path in sources:
    for line in open(path, encoding="utf-8", errors="replace"):
        if line.lstrip().startswith("#"):
            continue
        for m in re.finditer(r"__shared__\s+(?:__attribute__\(\([^()]*(?:\([^()]*\))?[^()]*\)\)\s+)?[\w:]+\s+([^;]+);", line):
            decl = re.sub(r"\[[^\]]*\]", "", m.group(1))
            names.update(d.strip().split()[-1] for d in decl.split(",") if d.strip())
out = subprocess.run(["nm", "-S", "-C", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
syms, begin, end = [], None, None
for line in out.splitlines():
    f = line.split(None, 3)
    if len(f) == 3 and f[2] in ("hipemu_lds_begin", "hipemu_lds_end"):
        if f[2] == "hipemu_lds_begin": begin = int(f[0], 16)
        else: end = int(f[0], 16)
    elif len(f) == 4 and f[3].startswith("dw::"):
        syms.append((int(f[0], 16), int(f[1], 16), f[2], f[3]))
if begin is None or end is None:
    sys.exit(f"check_lds: {lib} has no hipemu_lds_begin / hipemu_lds_end")
bad = []
shared = [s for s in syms if s[2] in "bBuV" and s[3].rsplit("::", 1)[-1] in names and "(" in s[3]]
for a, n, t, nm in shared:
    if not (begin <= a and a + n <= end):
        bad.append(f"__shared__ outside the poisoned range: {nm}")
for a, n, t, nm in syms:
    if begin <= a < end and (a, n, t, nm) not in shared:
        bad.append(f"not a __shared__ object, inside the poisoned range: {nm}")
if not shared or bad:
    sys.exit("check_lds: " + ("; ".join(bad) if bad else f"no __shared__ object found in {lib}"))
print(f"check_lds: {len(shared)} __shared__ objects, {sum(s[1] for s in shared)} bytes, in a {end - begin}-byte poisoned range")
