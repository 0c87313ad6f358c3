"""The list decoder's leaf penalty as the lane-per-path kernel evaluates it (es_softplus_dev.h: es_leaf_softplus_sl_sh -- the
straight-line softplus with its range flag --, the generic softplus where the flag is set, es_leaf_penalty) against es_math.h's
es_metric_penalty, compiled on the host: bit for bit, for both bit values, at every edge of the straight-line form and on a
million random leaf LLRs; the flag is set exactly outside |lam| < 512."""
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
/* (leaf LLR, bit) pairs whose penalty differs from es_metric_penalty's, or whose range flag is not !(|lam| < 512); *ncold: flags set */
long cmp_leaf(const double* lam, long n, long* first, long* ncold)
{
    long diff = 0; *first = -1; *ncold = 0;
    for (long i = 0; i < n; ++i) {
        const double al = __builtin_fabs(lam[i]);
        const uint32_t pref = (lam[i] >= 0.0) ? 1u : 0u;
        int bad = 0;
        double lp = es_leaf_softplus_sl_sh(al, tab, &bad, es_shift_reg());
        int same = (bad == !(al < 512.0));
        if (bad) { lp = es_softplus_neg_generic(-al, tab); ++*ncold; }          /* the kernel's cold path */
        for (uint32_t bit = 0; bit < 2; ++bit) {
            const double got = es_leaf_penalty(lp, al, pref, bit), want = es_metric_penalty(lam[i], bit, tab);
            same &= !memcmp(&got, &want, 8);
        }
        if (!same) { if (*first < 0) *first = i; ++diff; }
    }
    return diff;
}
"""


@pytest.fixture(scope="module")
def leaf_lib(tmp_path_factory):
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no host C compiler")
    d = tmp_path_factory.mktemp("leaf_penalty_dev")
    src, lib = d / "leaf.c", d / "libleaf.so"
    src.write_text(_DRIVER)
    # -ffp-contract=off: every rounding written out, as the oracle and the kernels build es_math.h
    subprocess.check_call([cc, "-O2", "-std=c11", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC",
                           "-I", CSRC, str(src), "-o", str(lib)])
    m = ctypes.CDLL(str(lib))
    m.cmp_leaf.restype = ctypes.c_long
    m.cmp_leaf.argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.POINTER(ctypes.c_long), ctypes.POINTER(ctypes.c_long)]
    return m


def _run(m, lam):
    lam = np.ascontiguousarray(lam, np.float64)
    first, ncold = ctypes.c_long(), ctypes.c_long()
    diff = m.cmp_leaf(lam.ctypes.data, lam.size, ctypes.byref(first), ctypes.byref(ncold))
    return diff, ncold.value, ("" if diff == 0 else f" first at lam={lam[first.value]!r} ({lam[first.value].hex()})")


def test_leaf_penalty_edges_bits(leaf_lib):
    sp = np.nextafter
    k0 = np.log(np.sqrt(2.0) - 1.0)                                   # exp(-|lam|) crosses sqrt(2) - 1: log1p's k == 0 / k == 1 split
    mags = np.array([0.0, 5e-324, 2.2250738585072014e-308, sp(2.2250738585072014e-308, 0.0), 1e-310, 2.0 ** -1074, 2.0 ** -1030,
                     2.0 ** -54, 2.0 ** -53, 2.0 ** -30, sp(2.0 ** -30, 0.0), sp(2.0 ** -30, 1.0), 2.0 ** -20, sp(2.0 ** -20, 0.0),
                     sp(2.0 ** -20, 1.0), -k0, sp(-k0, 0.0), sp(-k0, 1.0), 20.101268236238414, 37.5,
                     sp(512.0, 0.0), 511.99999999999994, 511.999, 512.0, sp(512.0, 1e3), 600.0, 745.2, 1e4, np.inf])
    lam = np.concatenate([mags, -mags])                               # +0 and -0, both signs of everything else
    diff, ncold, where = _run(leaf_lib, lam)
    assert diff == 0, f"{diff} leaf LLRs differ;{where}"
    assert ncold == 2 * int((mags >= 512.0).sum()) and ncold >= 10   # 512 and beyond took the cold path, 511.999... did not


def test_leaf_penalty_random_bits(leaf_lib):
    rng = np.random.default_rng(707)
    lam = rng.uniform(-40.0, 40.0, 1_000_000)
    diff, ncold, where = _run(leaf_lib, lam)
    assert diff == 0, f"{diff} of {lam.size} leaf LLRs differ;{where}"
    assert ncold == 0
