"""The device form of the list decoder's f (es_softplus_dev.h, as the lane-per-path kernel's hot loops run it: exp table at LDS
address 0, guard-free division) against es_math.h's es_polar_f_fast_sp compiled on the host, bit for bit."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "echoseal_amd", "csrc")

_HOST = r"""
#include "es_math.h"
static const uint64_t tab[ES_EXP_TAB_WORDS] = ES_EXP_TAB_INIT;
void eval_pairs(const double* a, const double* b, long n, double* out, int* bad)
{
    for (long i = 0; i < n; ++i) {
        int bd = 0;
        out[i] = es_polar_f_fast_sp(a[i], b[i], tab, &out[n + i], &out[2 * n + i], &bd);
        bad[i] = bd;
    }
}
"""


def _host_lib(d):
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no host C compiler")
    src, lib = d / "host_f.c", d / "libhost_f.so"
    src.write_text(_HOST)
    subprocess.check_call([cc, "-O2", "-std=c11", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC",
                           "-I", CSRC, str(src), "-o", str(lib)])
    m = ctypes.CDLL(str(lib))
    m.eval_pairs.restype = None
    m.eval_pairs.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p]
    return m


@pytest.mark.gpu
def test_device_polar_f_dev_bits(engine, tmp_path):
    import torch
    from test_softplus_dev import edge_t
    rng = np.random.default_rng(507)
    t = edge_t(rng)
    u = rng.permutation(t)
    n = 500_000
    llr = lambda k: np.clip(rng.normal(0, 6, k), -12, 12)
    a = np.concatenate([(t + u) / 2, t, llr(n), llr(n) + llr(n), rng.normal(0, 30, n), rng.uniform(-300, 300, n),
                        np.ldexp(rng.uniform(-1, 1, n), -rng.integers(0, 60, n))])
    b = np.concatenate([(u - t) / 2, np.zeros_like(t), llr(n), llr(n) - llr(n), rng.normal(0, 30, n), rng.uniform(-300, 300, n),
                        np.ldexp(rng.uniform(-1, 1, n), -rng.integers(0, 60, n))])
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    want = np.empty((3, a.size)); want_bad = np.empty(a.size, np.int32)
    _host_lib(tmp_path).eval_pairs(a.ctypes.data, b.ctypes.data, a.size, want.ctypes.data, want_bad.ctypes.data)
    got, got_bad = engine.polar_f(torch.from_numpy(a).to(engine.device), torch.from_numpy(b).to(engine.device))
    torch.cuda.synchronize()
    got = got.cpu().numpy(); got_bad = got_bad.cpu().numpy()
    assert np.array_equal(got_bad, want_bad)
    assert 0 < want_bad.sum() < a.size
    ok = want_bad == 0
    for k in range(3):
        assert np.array_equal(got[k, ok].view(np.uint64), want[k, ok].view(np.uint64)), f"row {k} differs"
