"""es_softplus_dev.h after the integer work came out of its two softplus halves (scale bits as one 32-bit shift-add on the high word,
the corner as one compare that also admits u == 2, kc over the zero low word of ES_EXP_SHIFT, the range flag taken from the operands):
every form -- es_softplus_neg_sl, es_polar_f_sl_sp, es_polar_f_sl, es_polar_f_slg -- against es_math.h's es_softplus_neg_fast /
es_polar_f_fast_sp / es_polar_f on the host, bit for bit (uint64 view), at every edge those rewrites touch."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_softplus_dev import edge_t

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "echoseal_amd", "csrc")

_DRIVER = r"""
#include <string.h>
#include "es_softplus_dev.h"
static const uint64_t tab[ES_EXP_TAB_WORDS] = ES_EXP_TAB_INIT;
static int same_bits(double x, double y) { return !memcmp(&x, &y, 8); }

/* f: the flag of the three straight-line forms; in range their value and softplus pair; for EVERY pair es_polar_f_slg against es_polar_f */
long cmp_f(const double* a, const double* b, long n, long* first, long* nbad)
{
    long diff = 0; *first = -1; *nbad = 0;
    for (long i = 0; i < n; ++i) {
        double s0, s1, t0, t1; int b0 = 0, b1 = 0, b2 = 0;
        const double x = es_polar_f_fast_sp(a[i], b[i], tab, &s0, &s1, &b0);
        const double y = es_polar_f_sl_sp(a[i], b[i], tab, &t0, &t1, &b1);
        const double z = es_polar_f_sl(a[i], b[i], tab, &b2);
        int same = (b0 == b1) && (b0 == b2) && same_bits(es_polar_f(a[i], b[i], tab), es_polar_f_slg(a[i], b[i], tab));
        if (same && !b0) same = same_bits(x, y) && same_bits(x, z) && same_bits(s0, t0) && same_bits(s1, t1);
        if (!same) { if (*first < 0) *first = i; ++diff; }
        *nbad += b0;
    }
    return diff;
}

/* the softplus alone: the flag, and in range the value; hu[i] = high word of u = 1 + exp(t) as the straight-line form sees it */
long cmp_sp(const double* t, long n, long* first, unsigned* hu)
{
    long diff = 0; *first = -1;
    for (long i = 0; i < n; ++i) {
        int k0, k1;
        const double x = es_softplus_neg_fast(t[i], tab, &k0);
        const double y = es_softplus_neg_sl(t[i], tab, &k1);
        if (k0 != k1 || (k0 && !same_bits(x, y))) { if (*first < 0) *first = i; ++diff; }
        hu[i] = (unsigned)es_hi32(1.0 + es_exp(t[i], tab));
    }
    return diff;
}

/* the scale bits for k = k_lo .. k_hi (ki = the bits of ES_EXP_SHIFT + k, as the fma leaves them): te1 + (ki << 45) against the high-word form */
long cmp_scale(long k_lo, long k_hi)
{
    long diff = 0;
    for (long k = k_lo; k <= k_hi; ++k) {
        const uint64_t ki = es_d2u(ES_EXP_SHIFT + (double)k);
        const uint64_t te1 = tab[2u * (uint32_t)(ki & 127u) + 1];
        const uint64_t want = te1 + (ki << 45);
        const uint64_t got = es_d2u(es_words2d((uint32_t)te1, es_scale_hi((uint32_t)(te1 >> 32), (uint32_t)ki)));
        diff += want != got;
    }
    return diff;
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no host C compiler")
    d = tmp_path_factory.mktemp("softplus_sl")
    src, so = d / "cmp.c", d / "libcmp.so"
    src.write_text(_DRIVER)
    subprocess.check_call([cc, "-O2", "-std=c11", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC",
                           "-I", CSRC, str(src), "-o", str(so)])
    m = ctypes.CDLL(str(so))
    m.cmp_f.restype = ctypes.c_long
    m.cmp_f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.POINTER(ctypes.c_long), ctypes.POINTER(ctypes.c_long)]
    m.cmp_sp.restype = ctypes.c_long
    m.cmp_sp.argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.POINTER(ctypes.c_long), ctypes.c_void_p]
    m.cmp_scale.restype = ctypes.c_long
    m.cmp_scale.argtypes = [ctypes.c_long, ctypes.c_long]
    return m


def run_f(m, a, b):
    a = np.ascontiguousarray(a, np.float64)
    b = np.ascontiguousarray(b, np.float64)
    first, nbad = ctypes.c_long(), ctypes.c_long()
    diff = m.cmp_f(a.ctypes.data, b.ctypes.data, a.size, ctypes.byref(first), ctypes.byref(nbad))
    where = "" if diff == 0 else f" first at a={a[first.value]!r}, b={b[first.value]!r}"
    return diff, nbad.value, where


def run_sp(m, t):
    t = np.ascontiguousarray(t, np.float64)
    first = ctypes.c_long()
    hu = np.empty(t.size, np.uint32)
    diff = m.cmp_sp(t.ctypes.data, t.size, ctypes.byref(first), hu.ctypes.data)
    return diff, hu, "" if diff == 0 else f" first at t={t[first.value]!r}"


LN2N = np.log(2.0) / 128


def table_t():
    """every k = round(t * 128 / ln 2) the straight-line form serves (|t| < 512: k down to -94 548, so every table index hundreds of
    times, with every borrow pattern of ki's high bits), at the middle of its interval and next to both ends"""
    k = np.arange(-94_560, 1, dtype=np.float64)
    t = np.concatenate([k * LN2N, (k - 0.499) * LN2N, (k + 0.499) * LN2N])
    return t[t <= 0]                                  # the softplus argument is -|x|


def corner_t():
    """t at which u = 1 + exp(t) steps from one high word to the next, 0x3FFFFFFB|C .. 0x3FFFFFFF|0x40000000: u = 2 - m * 2^-20, both
    sides of each step in steps of the spacing of y there (2^-53), and t == 0 itself"""
    j = np.arange(-3000, 3001) * 2.0 ** -54
    t = np.concatenate([np.log1p(-m * 2.0 ** -20) + j for m in range(0, 6)])
    return np.concatenate([t[t <= 0], [0.0, -0.0, -5e-324, -2.0 ** -54, -2.0 ** -53, -1.1e-16, -1.2e-16]])


def edge_pairs(rng):
    """pairs whose difference and sum land on the edges (a = (t1 + t2) / 2, b = (t2 - t1) / 2, mirrored and with a zero operand), a == b,
    a == -b, and pairs clipped to +-12"""
    t = np.concatenate([edge_t(rng)[::8], table_t()[::3], corner_t(),
                        -np.array([np.nextafter(512.0, 0.0), 512.0, np.nextafter(512.0, np.inf), 511.999, 512.001, 1000.0])])
    u = rng.permutation(t)
    z = np.zeros_like(t)
    v = np.concatenate([rng.uniform(-12, 12, 20_000), [12.0, -12.0, 0.0, 5e-324, 2.0 ** -30, 256.0, 255.99999999999997, 256.00000000000006, 300.0]])
    c = rng.choice([-12.0, 12.0], v.size)
    a = np.concatenate([(t + u) / 2, (u - t) / 2, t, z, v, v, c, c, v, c])
    b = np.concatenate([(u - t) / 2, (t + u) / 2, z, t, v, -v, c, -c, c, v])
    return a, b


def test_scale_bits_every_index_both_signs(lib):
    assert lib.cmp_scale(-95_000, 95_000) == 0


def test_softplus_sl_table_and_corner_bits(lib):
    t = np.concatenate([table_t(), corner_t()])
    diff, hu, where = run_sp(lib, t)
    assert diff == 0, f"{diff} softplus values differ;{where}"
    for w in range(0x3FFFFFFB, 0x40000001):          # both sides of every step of the corner test, u == 2 included
        assert (hu == w).any(), hex(w)


def test_softplus_sl_edges_bits(lib):
    rng = np.random.default_rng(701)
    t = np.concatenate([edge_t(rng), -np.array([np.nextafter(512.0, 0.0), 512.0, np.nextafter(512.0, np.inf)])])
    diff, _, where = run_sp(lib, t)
    assert diff == 0, f"{diff} softplus values differ;{where}"


def test_f_forms_edge_pairs_bits(lib):
    a, b = edge_pairs(np.random.default_rng(702))
    diff, nbad, where = run_f(lib, a, b)
    assert diff == 0, f"{diff} of {a.size} pairs differ;{where}"
    assert nbad > 0


def test_f_forms_tree_depth_scales_bits(lib):
    """four million pairs at the scales of tree depths 1..10: channel LLRs clipped to +-12 at depth 1, then what f (magnitudes
    shrink towards min(|a|, |b|), down to ~x*y/2) and g (sums: magnitudes double) leave level by level"""
    rng = np.random.default_rng(703)
    n = 200_000
    aa, bb = [], []
    for d in range(10):
        for scale in (6.0 * 2.0 ** -d, 6.0 * 2.0 ** min(d, 5)):
            aa.append(np.clip(rng.normal(0, scale, n), -12 * 2.0 ** d, 12 * 2.0 ** d))
            bb.append(np.clip(rng.normal(0, scale, n), -12 * 2.0 ** d, 12 * 2.0 ** d))
    a, b = np.concatenate(aa), np.concatenate(bb)
    assert a.size >= 4_000_000
    diff, _, where = run_f(lib, a, b)
    assert diff == 0, f"{diff} of {a.size} pairs differ;{where}"
