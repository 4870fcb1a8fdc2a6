#!/usr/bin/env python3
"""Records tests/golden/gzip_members.json: length and sha256 of the gzip members k_gzip makes of the named inputs of tests/gzip_stream.py, from the
kernel's source on the CPU emulation (tests/emu).  tests/test_emu_gzip_stream.py and tests/test_gpu_gzip_stream.py compare against it: the device
must make the emulation's bytes.  Run it again, on purpose, after a change of the coder:   python3 tests/golden/make_gzip_members.py"""
import json, os, subprocess, sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import gzip_stream as G
from dwgsim_amd import api

subprocess.run([os.path.join(HERE, "..", "emu", "build.sh")], check=True, stdout=subprocess.DEVNULL)
session = G.Session(api.load(os.path.join(HERE, "..", "emu", "libdwgsim_emu.so")), HERE)
doc = {"what": "gzip members of the named inputs of tests/gzip_stream.py, made by dw_gzip.hip on the CPU emulation: bytes of text, bytes and sha256 of the members",
       "members": G.golden_digests(session)}
session.close()
with open(G.GOLDEN_FILE, "w") as f:
    json.dump(doc, f, indent=1, sort_keys=True)
    f.write("\n")
print("wrote", G.GOLDEN_FILE, len(doc["members"]), "inputs")
