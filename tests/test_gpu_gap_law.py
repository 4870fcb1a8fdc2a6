"""The gap draw on the device, on EVERY 32-bit word (dwgsim_hip_selftest_gap: the product's geom_gap with its own table and reciprocal, the table staged
in LDS as k_simulate stages it), against the oracle's boundaries (exact parity of the primitive) and against the exact geometric law (tests/gap_law.py,
bounds derived in DESIGN.md "The law of the gap draw").  Prints the measured maxima next to the bounds."""
import ctypes as C

import numpy as np
import pytest

import gap_law as L
from dwgsim_amd import api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    lib = api.load()
    lib.dwgsim_hip_selftest_gap.argtypes = [C.c_int, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint64)]
    lib.dwgsim_hip_selftest_gap.restype = C.c_int
    return lib


@pytest.fixture(scope="module")
def olib(oracle_bin):
    return L.oracle()


@pytest.mark.parametrize("thr", L.THRESHOLDS, ids=hex)
def test_gap_draw_on_every_word(lib, olib, thr):
    report = []
    for lo, cnt in L.windows(olib, thr):
        chg = np.zeros(cnt, dtype=np.uint32)
        out = (C.c_uint64 * 4)()
        assert lib.dwgsim_hip_selftest_gap(0, thr, 0, 1 << 32, lo, cnt, chg.ctypes.data, out) == 0
        assert out[2] == 1 << 32 and out[0] == 0, list(out)            # every word, and G never increases with w
        B = chg.astype(np.int64)
        B[np.arange(lo, lo + cnt) <= out[3]] = 1 << 32                  # g <= G(2^32 - 1): every word has G >= g
        # 1. the change points are the oracle's boundaries, for every g
        want = L.oracle_bounds(olib, thr, lo, cnt)
        bad = np.nonzero(B != want)[0]
        assert bad.size == 0, (thr, [(lo + int(k), int(B[k]), int(want[k])) for k in bad[:5]])
        # 2. the tail law below the clip
        excess, rel, absmax = L.tail_deviation(thr, lo, B)
        assert excess <= 0, (thr, lo, excess)
        report.append(f"tail |B - B*| <= {absmax:.0f} words, {rel:.3g} B* where B* > 1e6 (bound {L.EPS} B* + {L.K_WORDS})")
        # 3. the per-position marginal over a read end staged in LDS and over a walk window
        if lo == 1 and thr > 3:
            u = L.per_position(thr, B)
            ex1200, r1200 = L.per_position_excess(thr, u)
            ex256, r256 = L.per_position_excess(thr, u[:256])
            assert ex1200 <= 0 and ex256 <= 0, (thr, r1200, r256)
            report.append(f"per position |u_i - e'| <= {r1200:.3g} e' (i < 1200), {r256:.3g} e' (i < 256) (bound {L.ETA} e' + 2^-25)")
        # 4. the clip: only where G* is at least 2^30 - 1 - 2^14, on #{G* >= 2^30 - 1} words within the tail bound
        if lo + cnt == L.CLIP + 1:
            clipped = int(out[1])
            assert clipped == B[-1]
            ex = L.exact_tail(thr, [L.CLIP])[0]
            assert abs(clipped - ex) <= L.EPS * ex + L.K_WORDS and clipped <= L.exact_tail(thr, [L.CLIP - 2 ** 14])[0]
            report.append(f"clip on {clipped} words ({clipped / 2 ** 32:.1%}), G* >= 2^30 - 1 on {ex:.0f}")
        elif lo == 1 and lo + cnt <= L.CLIP:
            assert (out[1] == 0) == (len(L.windows(olib, thr)) == 1)    # a window up to one past G(0) below the clip: nothing clips
    print(f"\nthr {thr:#x} (e' = {thr / 2 ** 32:.3g}): " + "; ".join(report))
