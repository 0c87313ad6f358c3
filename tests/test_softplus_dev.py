"""es_softplus_dev.h (the list decoder's f with fewer vector instructions) against es_math.h's es_polar_f_fast_sp, compiled on
the host: the value, both softplus terms and the range flag, bit for bit, on ten million operand pairs and every edge of the
straight-line form's selects."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "echoseal_amd", "csrc")

_DRIVER = r"""
#include <string.h>
#include "es_softplus_dev.h"
static const uint64_t tab[ES_EXP_TAB_WORDS] = ES_EXP_TAB_INIT;
/* pairs whose flag, or (in range) value / softplus terms, differ; the first such index in *first */
long cmp_pairs(const double* a, const double* b, long n, long* first, long* nbad)
{
    long diff = 0; *first = -1; *nbad = 0;
    for (long i = 0; i < n; ++i) {
        double s0, s1, t0, t1; int b0 = 0, b1 = 0;
        const double x = es_polar_f_fast_sp(a[i], b[i], tab, &s0, &s1, &b0);
        const double y = es_polar_f_sl_sp(a[i], b[i], tab, &t0, &t1, &b1);
        int same = (b0 == b1);
        if (same && !b0) same = !memcmp(&x, &y, 8) && !memcmp(&s0, &t0, 8) && !memcmp(&s1, &t1, 8);
        if (!same) { if (*first < 0) *first = i; ++diff; }
        *nbad += b0;
    }
    return diff;
}
"""


@pytest.fixture(scope="module")
def cmp_lib(tmp_path_factory):
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no host C compiler")
    d = tmp_path_factory.mktemp("softplus_dev")
    src, lib = d / "cmp.c", d / "libcmp.so"
    src.write_text(_DRIVER)
    # -ffp-contract=off: every rounding written out, as the oracle and the kernels build es_math.h
    subprocess.check_call([cc, "-O2", "-std=c11", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC",
                           "-I", CSRC, str(src), "-o", str(lib)])
    m = ctypes.CDLL(str(lib))
    m.cmp_pairs.restype = ctypes.c_long
    m.cmp_pairs.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.POINTER(ctypes.c_long),
                            ctypes.POINTER(ctypes.c_long)]
    return m


def _run(m, a, b):
    a = np.ascontiguousarray(a, np.float64)
    b = np.ascontiguousarray(b, np.float64)
    first, nbad = ctypes.c_long(), ctypes.c_long()
    diff = m.cmp_pairs(a.ctypes.data, b.ctypes.data, a.size, ctypes.byref(first), ctypes.byref(nbad))
    where = "" if diff == 0 else f" first at a={a[first.value]!r}, b={b[first.value]!r}"
    return diff, nbad.value, where


def edge_t(rng):
    """softplus arguments t <= 0 at every edge of the straight-line form"""
    sp = np.nextafter
    t = np.concatenate([
        np.array([0.0, -0.0, -2.0 ** -54, -2.0 ** -55, -2.0 ** -53, -5e-324, -1e-300,
                  -1.1e-16, -2.86e-6, -0.8813735870195429, -0.881373587019543, -0.8813735870195432,
                  -20.1, -20.101268236238414, -20.101268236238418, -37.42994775023705, -37.5,
                  -511.9, -sp(512.0, 0.0), -512.0, -sp(512.0, np.inf), -600.0, -745.2]),
        -np.ldexp(rng.uniform(0.5, 1, 400_000), -rng.integers(40, 70, 400_000)),          # |t| around 2^-54
        -(10.0 ** rng.uniform(-16.5, -5, 400_000)),                                       # log1p's |f| < 2^-20 corner ...
        -(1.1e-16 + rng.uniform(-5e-17, 5e-17, 200_000)), -(2.86e-6 + rng.uniform(-5e-8, 5e-8, 200_000)),   # ... and its edges
        -rng.uniform(0.86, 0.90, 400_000), -(0.8813735870195430 + rng.integers(-2000, 2000, 100_000) * 2.0 ** -53),   # sqrt2 - 1
        -rng.uniform(19.5, 20.7, 400_000), -(20.101268236238415 + rng.integers(-2000, 2000, 100_000) * 2.0 ** -48),   # 2^-29
        -rng.uniform(500, 520, 200_000), -(512.0 + rng.integers(-2000, 2000, 100_000) * 2.0 ** -43),               # 512
    ])
    return t


def test_softplus_dev_edges_bits(cmp_lib):
    """pairs whose difference AND sum land on the edges: a = (t1 + t2) / 2, b = (t2 - t1) / 2 (and the mirrored pair)"""
    rng = np.random.default_rng(505)
    t = edge_t(rng)
    u = rng.permutation(t)
    a, b = (t + u) / 2, (u - t) / 2
    diff, _, where = _run(cmp_lib, np.concatenate([a, b, t, np.zeros_like(t)]), np.concatenate([b, a, np.zeros_like(t), t]))
    assert diff == 0, f"{diff} pairs differ;{where}"


def test_softplus_dev_bulk_bits(cmp_lib):
    """ten million pairs the decoder produces: +-12-clipped channel LLRs, their sums and differences down the tree, equal and
    opposite operands, a grid of clipped values, wide and tiny magnitudes"""
    rng = np.random.default_rng(506)
    n = 1_250_000
    llr = lambda k: np.clip(rng.normal(0, 6, k), -12, 12)
    grid = np.arange(-12.0, 12.0 + 1 / 64, 1 / 64)
    a = np.concatenate([
        llr(n), llr(n) + llr(n), rng.normal(0, 30, n), np.ldexp(rng.uniform(-1, 1, n), -rng.integers(0, 60, n)),
        rng.choice(grid, n), np.clip(rng.normal(0, 6, n), -12, 12), rng.uniform(-300, 300, n), rng.normal(0, 1, n)])
    b = np.concatenate([
        llr(n), llr(n) - llr(n), rng.normal(0, 30, n), np.ldexp(rng.uniform(-1, 1, n), -rng.integers(0, 60, n)),
        rng.choice(grid, n), np.where(rng.random(n) < 0.5, 1.0, -1.0) * a[5 * n:6 * n] * (1 + rng.integers(-1, 2, n) * 2.0 ** -52),
        rng.uniform(-300, 300, n), rng.normal(0, 1, n) * 1e-3])
    assert a.size >= 10_000_000
    diff, nbad, where = _run(cmp_lib, a, b)
    assert diff == 0, f"{diff} of {a.size} pairs differ;{where}"
    assert nbad > 0                                   # the range flag was exercised as well
