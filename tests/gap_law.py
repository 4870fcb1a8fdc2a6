"""The law of the gap draw G = geom_gap(w) (dwgsim_amd/csrc/dw_common.hpp) against the ideal draw G* = floor(-log2 U / -log2(1 - e')), U = (2 w + 1) / 2^33,
e' = thr / 2^32 -- shared by tests/test_gap_law.py (the oracle's copy by bisection, the emulated product near its boundaries) and tests/test_gpu_gap_law.py
(the product on the device, every 32-bit word).  The bounds are derived in DESIGN.md "The law of the gap draw".

A gap function is described by its BOUNDARIES B(g) = #{w : G(w) >= g}: G is non-increasing in w, so B(g) is also the first word whose G is below g."""
import ctypes as C
import math
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIP = 0x3FFFFFFF
EPS, K_WORDS = 2e-6, 2                  # tail:         |B(g) - B*(g)| <= EPS B*(g) + K_WORDS, every g below the clip
ETA, QUANT = 2e-3, 2.0 ** -25           # per position: |u_i - e'| <= ETA e' + QUANT, i < 1200 (a read end staged in LDS) and i < 256 (a walk window)
HORIZON = 1200


def thr_of(e):
    return math.ceil(e * 2 ** 32)       # the product's threshold of a rate (dw_host.cpp, -e / -r / -R)


SATURATING = [2 ** 32 - 2 ** (32 - 2 ** k) for k in range(6)]     # -log2(1 - e') = 1, 2, 4, 8, 16, 32: 2^31, 3 2^30, ..., 2^32 - 1
THRESHOLDS = ([1, 2, 3] + [thr_of(e) for e in (1e-6, 1e-4, 1e-3, 0.01, 0.02, 0.05, 0.1, 0.2, 0.3)]
              + sorted({t + d for t in SATURATING for d in (-1, 0, 1) if t + d < 2 ** 32}))


def oracle(path=None):
    lib = C.CDLL(path or os.path.join(ROOT, "oracle", "build", "liboracle.so"))
    lib.oracle_gap_bounds.argtypes = [C.c_uint64, C.c_uint32, C.c_uint64, C.c_void_p]
    lib.oracle_gap_bounds.restype = None
    lib.oracle_flow_gap.argtypes = [C.c_uint64, C.c_uint32]
    lib.oracle_flow_gap.restype = C.c_uint32
    lib.oracle_flow_gap_params.argtypes = [C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_int32)]
    lib.oracle_flow_gap_params.restype = None
    return lib


def oracle_bounds(lib, thr, g_lo, g_cnt):
    out = np.zeros(g_cnt, dtype=np.uint64)
    lib.oracle_gap_bounds(thr, g_lo, g_cnt, out.ctypes.data)
    return out.astype(np.int64)


def windows(lib, thr, cap=1 << 25, win=1 << 22):
    """the g ranges [g_lo, g_lo + g_cnt) a test looks at: every g from 1 to one past G(0), or -- where G(0) is at the clip and the values are too many -- the
    first `win` values and the last `win` below the clip (thr = 1, 2, 3: 78 %, 61 %, 47 % of the words clip)"""
    top = min(lib.oracle_flow_gap(thr, 0), CLIP) + 1
    return [(1, top)] if top <= cap else [(1, win), (CLIP + 1 - win, win)]


def exact_tail(thr, g):
    """B*(g) = #{w : G*(w) >= g} = floor((2^33 (1 - e')^g - 1) / 2) + 1 (0 where 2^33 (1 - e')^g < 1), in long double: |error| < 1e-6 of a word below
    2^33 (anchored against 50-digit values by tests/test_gap_law.py), so the floor can be off by one only where the exact value is within 1e-6 of an integer"""
    e = np.longdouble(thr) / np.longdouble(2 ** 32)
    x = np.ldexp(np.exp(np.asarray(g, dtype=np.longdouble) * np.log1p(-e)), 33)
    return np.where(x >= 1, np.floor((x - 1) / 2) + 1, 0).astype(np.float64)


def exact_tail_mp(thr, g, digits=50):
    import mpmath
    with mpmath.workdps(digits):
        x = mpmath.mpf(2) ** 33 * (1 - mpmath.mpf(thr) / 2 ** 32) ** g
        return mpmath.floor((x - 1) / 2) + 1 if x >= 1 else mpmath.mpf(0), x


def tail_deviation(thr, g_lo, B):
    """(largest |B(g) - B*(g)| - EPS B*(g) - K_WORDS: must be <= 0; largest |B - B*| / B* where B* > 10^6; largest |B - B*| in words)"""
    g = np.arange(g_lo, g_lo + len(B))
    ex = exact_tail(thr, g)
    d = np.abs(B.astype(np.float64) - ex)
    big = ex > 1e6
    return float(np.max(d - EPS * ex - K_WORDS)), float(np.max(d[big] / ex[big])) if big.any() else 0.0, float(np.max(d))


def per_position(thr, B, horizon=HORIZON):
    """u_i = P(some site of the chain S_0 = G_0, S_(m+1) = S_m + 1 + G_(m+1) is at i), i < horizon, exactly from the boundaries B(1), B(2), ... (B(0) = 2^32):
    P(G = k) = (B(k) - B(k + 1)) / 2^32, u_i = P(G = i) + sum_(k < i) u_k P(G = i - k - 1).  Returns u (float64; rounding far below the bounds)."""
    n = horizon
    Bf = np.concatenate([[2.0 ** 32], B[: n + 1].astype(np.float64), np.zeros(max(0, n + 1 - len(B)))])      # (B(g) = 0 beyond the last window entry, past G(0))
    p = (Bf[:-1] - Bf[1:]) * 2.0 ** -32
    u = np.zeros(n)
    for i in range(n):
        u[i] = p[i] + (np.dot(u[:i], p[i - 1::-1]) if i else 0.0)
    return u


def per_position_excess(thr, u):
    """largest |u_i - e'| - (ETA e' + QUANT) (must be <= 0) and largest |u_i - e'| / e'"""
    e = thr * 2.0 ** -32
    d = np.abs(u - e)
    return float(np.max(d - ETA * e - QUANT)), float(np.max(d) / e)


# ---- the integer quotient the reciprocal stands for: G_int = floor(Lu / Lq), Lu and Lq as in dw_kernels.hpp / dw_common.hpp (Python integers, no rounding) ----
def _ilog2_fixed(y, fb):
    p = y.bit_length() - 1
    m, frac = y << (63 - p), 0
    for _ in range(fb):
        sq = m * m
        if sq >> 127:
            m, frac = sq >> 64, (frac << 1) | 1
        else:
            m, frac = sq >> 63, frac << 1
    return (p << fb) | frac


LG = [_ilog2_fixed(256 + i, 32) & 0xFFFFFFFF for i in range(256)] + [2 ** 32 - 1]      # floor(2^32 log2(1 + i / 256))


def g_int(thr, w):
    X = 2 * w + 1
    p = X.bit_length() - 1
    M = X << (63 - p)
    idx, r16 = (M >> 55) & 0xFF, (M >> 39) & 0xFFFF
    f = LG[idx] + (((LG[idx + 1] - LG[idx]) * r16) >> 16)
    Lu = ((33 - p) << 56) - (f << 24)
    Lq = (32 << 56) - _ilog2_fixed(2 ** 32 - thr, 56)
    return min(Lu // Lq, CLIP)


def g_int_bounds(thr, g_max):
    """B_int(g) for g = 1 .. g_max by bisection"""
    out = []
    for g in range(1, g_max + 1):
        lo, hi = 0, 2 ** 32
        while lo < hi:
            m = (lo + hi) // 2
            if g_int(thr, m) >= g:
                lo = m + 1
            else:
                hi = m
        out.append(lo)
    return np.array(out, dtype=np.int64)
