"""CPU-only: the law of the gap draw (dw_common.hpp geom_gap; DESIGN.md "The law of the gap draw").  The parity suites compare the kernels with the
oracle's flow_gap, the same integer code written out again; here both are held against the exact geometric law G* = floor(-log2 U / -log2(1 - e')),
U = (2 w + 1) / 2^33, computed in high precision -- the oracle's function through its boundaries (bisection), and the product's own source, compiled
for the CPU emulation, on the words next to every boundary.  tests/test_gpu_gap_law.py does the same on the device for every 32-bit word."""
import ctypes as C
import os, random, subprocess

import numpy as np
import pytest

import gap_law as L
from dwgsim_amd import api
from parity_common import compare_case

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def olib(oracle_bin):
    return L.oracle()


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.run([os.path.join(HERE, "emu", "build.sh")], check=True, stdout=subprocess.DEVNULL)
    lib = api.load(os.path.join(HERE, "emu", "libdwgsim_emu.so"))
    lib.dwgsim_hip_selftest_gap.argtypes = [C.c_int, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint64)]
    lib.dwgsim_hip_selftest_gap.restype = C.c_int
    return lib


def test_long_double_reference_agrees_with_50_digits():
    """the dense reference (long double) against mpmath at 50 digits, at every tested threshold: the values agree to 1e-6 of a word"""
    for thr in L.THRESHOLDS:
        gs = sorted({1, 2, 3, 17, 1000, 123457, 2 ** 22, 2 ** 30 - 1} | {int(x) for x in np.geomspace(1, 40 / (thr * 2.0 ** -32), 12)})
        ld = np.ldexp(np.exp(np.asarray(gs, dtype=np.longdouble) * np.log1p(-np.longdouble(thr) / 2 ** 32)), 33)
        for g, x in zip(gs, ld):
            fl, xm = L.exact_tail_mp(thr, g)
            assert abs(float(xm - float(x)) if xm < 2 ** 60 else 0.0) < 1e-6 * max(1.0, float(xm) * 2 ** -33), (thr, g)
            if abs(float(xm) - round(float(xm))) > 1e-5 or float(xm) < 1:
                assert L.exact_tail(thr, [g])[0] == float(fl), (thr, g)


def law_bounds(olib, thr):
    """every window of g the law is checked on, with the oracle's boundaries: [(g_lo, B)]"""
    return [(lo, L.oracle_bounds(olib, thr, lo, cnt)) for lo, cnt in L.windows(olib, thr, cap=1 << 21, win=1 << 20)]


@pytest.mark.parametrize("thr", L.THRESHOLDS, ids=hex)
def test_tail_law_of_the_oracle_gap(olib, thr):
    """|#{w : G(w) >= g} - #{w : G*(w) >= g}| <= EPS #{G* >= g} + K_WORDS for every g below the clip (thr 1e-6 and below: the first and the last
    2^20 values below it).  (B(g) = 2^32 up to G(2^32 - 1): 0, but 128 / 64 / 42 at thr = 1 / 2 / 3, where one step of the 25 bits of U the draw
    resolves in [1/2, 1) is 128 / 64 / 42 gap values)"""
    assert olib.oracle_flow_gap(thr, 0xFFFFFFFF) == ({1: 128, 2: 64, 3: 42}.get(thr, 0))
    worst = []
    for lo, B in law_bounds(olib, thr):
        assert np.all(np.diff(B) <= 0)
        excess, rel, absmax = L.tail_deviation(thr, lo, B)
        assert excess <= 0, (thr, lo, excess)
        worst.append((rel, absmax))
    print(f"thr {thr:#x}: tail |B - B*| <= {max(w[1] for w in worst):.0f} words, <= {max(w[0] for w in worst):.3g} B* where B* > 1e6 (bound {L.EPS} B* + {L.K_WORDS})")


@pytest.mark.parametrize("thr", [t for t in L.THRESHOLDS if t > 3], ids=hex)
def test_per_position_marginal_of_the_oracle_gap(olib, thr):
    """what the product promises: position i of a read end (i < 1200) or of a walk window (i < 256) is a site with probability e', within ETA e' + QUANT"""
    u = L.per_position(thr, L.oracle_bounds(olib, thr, 1, min(L.HORIZON + 1, olib.oracle_flow_gap(thr, 0) + 2)))
    excess, rel = L.per_position_excess(thr, u)
    assert excess <= 0, (thr, excess, rel)
    print(f"thr {thr:#x}: per-position |u_i - e'| <= {rel:.3g} e'")


@pytest.mark.parametrize("thr", [1, 2, 3])
def test_clip_of_the_oracle_gap(olib, thr):
    """G = 0x3FFFFFFF (the clip) on #{w : G* >= 2^30 - 1} words within the tail bound, and never where G* < 2^30 - 1 - 2^14; every consumer stops a chain
    far below: a walk window at 256, the flow ordinals of a read at FLOW_CAP_MAX = 2^20 bases, a read end at its length"""
    B = L.oracle_bounds(olib, thr, L.CLIP, 1)[0]
    ex = L.exact_tail(thr, [L.CLIP])[0]
    assert abs(B - ex) <= L.EPS * ex + L.K_WORDS
    assert B <= L.exact_tail(thr, [L.CLIP - 2 ** 14])[0]
    assert 0.4 < B / 2 ** 32 < 0.8
    assert max(256, 1 << 20) < L.CLIP - 2 ** 14


@pytest.mark.parametrize("thr", sorted({t + d for t in L.SATURATING for d in (-1, 0, 1) if t + d < 2 ** 32}), ids=hex)
def test_floor_semantics_at_saturating_thresholds(olib, thr):
    """Where -log2(1 - e') is a power of two the reciprocal is 2^64: the host passes it as 2^63 and one shift less, so that G is exactly
    floor(Lu / Lq) -- the quotient the reciprocal stands for -- at those thresholds and their neighbours, including G(0) = 33 at e' = 1/2"""
    g0 = olib.oracle_flow_gap(thr, 0)
    assert np.array_equal(L.oracle_bounds(olib, thr, 1, g0 + 1), L.g_int_bounds(thr, g0 + 1))
    assert g0 == L.g_int(thr, 0)
    if thr == 2 ** 31:
        assert g0 == 33


def test_floor_semantics_at_moderate_thresholds(olib):
    for thr in [L.thr_of(e) for e in (0.02, 0.05, 0.1, 0.3)]:
        g0 = olib.oracle_flow_gap(thr, 0)
        assert np.array_equal(L.oracle_bounds(olib, thr, 1, g0 + 1), L.g_int_bounds(thr, g0 + 1)), thr


@pytest.mark.parametrize("thr", [L.thr_of(e) for e in (0.3, 0.05, 0.02)] + L.SATURATING + [1, L.thr_of(1e-6), L.thr_of(1e-3)], ids=hex)
def test_product_source_at_the_oracle_boundaries_on_cpu_emulation(emu_lib, olib, thr):
    """dwgsim_hip_selftest_gap (the product's geom_gap, flow_gap_params and flow_log2_table, compiled by g++) on the words b - 2 .. b + 2 around every
    boundary b of the oracle's function (at the three smallest thresholds: 1500 boundaries drawn at random): the first word below g is b, and G does
    not increase there"""
    rnd = random.Random(thr)
    g0 = min(olib.oracle_flow_gap(thr, 0), L.CLIP)
    gs = list(range(1, g0 + 1)) if g0 <= 2000 else sorted(rnd.sample(range(1, g0 + 1), 1500))
    out = (C.c_uint64 * 4)()
    chg = np.zeros(1, dtype=np.uint32)
    for g in gs:
        b = int(L.oracle_bounds(olib, thr, g, 1)[0])
        first = min(max(b - 2, 0), 2 ** 32 - 5)
        assert emu_lib.dwgsim_hip_selftest_gap(0, thr, first, 5, g, 1, chg.ctypes.data, out) == 0
        assert out[0] == 0 and out[2] == 5, (thr, g, b, list(out))
        want = b if first < b < first + 5 else 0
        assert int(chg[0]) == want, (thr, g, b, int(chg[0]))


def test_product_source_on_a_whole_range_on_cpu_emulation(emu_lib, olib):
    """... and on 2^20 consecutive words at e' = 0.001 (the default -r): every change point the oracle has there"""
    thr, first, n = L.thr_of(1e-3), 3 << 30, 1 << 20
    lo, hi = olib.oracle_flow_gap(thr, first + n - 1), olib.oracle_flow_gap(thr, first)
    chg = np.zeros(hi - lo, dtype=np.uint32)
    out = (C.c_uint64 * 4)()
    assert emu_lib.dwgsim_hip_selftest_gap(0, thr, first, n, lo + 1, hi - lo, chg.ctypes.data, out) == 0
    assert out[0] == 0 and out[1] == 0 and out[2] == n
    assert np.array_equal(chg.astype(np.int64), L.oracle_bounds(olib, thr, lo + 1, hi - lo))


@pytest.mark.parametrize("flags", ["-z 5 -N 300 -1 60 -2 40 -e 0.5 -E 0.75", "-z 6 -N 300 -1 50 -2 50 -e 0.9375 -E 0.99609375 -y 0.1"])
def test_saturating_rates_end_to_end_on_cpu_emulation(emu_lib, oracle_bin, golden_dir, flags):
    """error rates whose thresholds saturated the reciprocal (2^31, 3 2^30, 2^32 - 2^28, 2^32 - 2^24): reads as the oracle's"""
    compare_case(emu_lib, oracle_bin, os.path.join(golden_dir, "tiny.fa"), flags, batch_pairs=200)
