"""The clips of the presence-map tests, shared by tests/test_presence_map_host.py and tests/test_gpu_presence_map.py: the
five-second clips A and B of tests/presence_cases.py with samples [96300, 96300 + 12650) removed -- ten frames and 500 samples, so the grid
anchor t = col + phase - 1215 ctr moves from -777 to -777 - 12650 --, the same clip resampled by 10001 / 10000, A's unmarked host, and
their correlation rows from the CPU oracle, each made once per session; and the folds that hold every edge of the device pick's definition
(include/echoseal_pick.h)."""
import functools

import numpy as np

import presence_cases as PC

SECONDS = 5.0
CUT_AT, CUT_LEN = 96_300, 12_650
SPAN = (0, 256)
FL = 1215
T0 = -PC.CUT                                             # the anchor before the cut; after it, T0 - CUT_LEN


@functools.lru_cache(maxsize=None)
def clip(kind: str, name: str = "A") -> np.ndarray:
    """kind: whole (marked, five seconds), spliced, drifted (spliced, then resampled by 10001 / 10000), unmarked (the host alone)."""
    if kind == "whole":
        x = PC.marked(name, seconds=SECONDS)
    elif kind == "spliced":
        w = clip("whole", name)
        x = np.concatenate([w[:CUT_AT], w[CUT_AT + CUT_LEN:]])
    elif kind == "drifted":
        from scipy.signal import resample_poly
        x = resample_poly(clip("spliced", name).astype(np.float64), 10001, 10000).astype(np.float32)
    elif kind == "unmarked":
        x = PC.host(name, SECONDS, unmarked=True)[PC.CUT:]
    else:
        raise KeyError(kind)
    x = np.ascontiguousarray(x, np.float32)
    x.setflags(write=False)
    return x


_ROWS: dict = {}


def rows(O, kind: str, name: str = "A"):
    """-> (corr float64 [4, n - 62], nlag) of clip(kind, name) from the CPU oracle, made once and left unchanged."""
    if (kind, name) not in _ROWS:
        corr, nlag = PC.oracle_rows(O, clip(kind, name))
        corr.setflags(write=False)
        _ROWS[kind, name] = (corr, nlag)
    return _ROWS[kind, name]


def edge_folds():
    """Folds [3, D, 1215] that hold every edge of the definition, by name."""
    rng = np.random.default_rng(26)
    out = {}
    for D in (1, 2, 5):
        out[f"random-D{D}"] = (rng.standard_normal((3, D, FL)), None)
    f = rng.standard_normal((3, 2, FL)); f[0, 1] = 0.75; f[1] = -3.0; f[2, 0, 7] = f[2, 1, 7] = f[2, 1, 3] = 9.0
    out["equal-values"] = (f, None)                                         # a row of equal values, a record of them, ties across rows
    f = -np.abs(rng.standard_normal((3, 2, FL))) - 1.0; f[0, 1, 5], f[0, 0, 9], f[0, 1, 2] = -0.0, 0.0, -0.0; f[1, 0, :4] = (0.0, -0.0, 0.0, -0.0)
    out["zeros-of-both-signs"] = (f, None)
    f = rng.standard_normal((3, 3, FL)); f[:, 1] = -np.inf; f[2, 0, 100:200] = -np.inf
    out["a-row-of-minus-infinity"] = (f, None)
    f = rng.standard_normal((3, 5, FL)); f[0, 2:] = np.nan; f[1, 4:] = np.nan; f[2] = np.nan
    out["nan-past-nwarp"] = (f, [2, 4, 0])
    out["nothing-to-pick"] = (np.concatenate([np.full((2, 2, FL), -np.inf), rng.standard_normal((1, 2, FL))]), [2, 1, 0])
    out["only-negative"] = (-np.abs(rng.standard_normal((3, 2, FL))) - 0.5, None)
    f = rng.standard_normal((3, 5, FL)); f[:, 4, 1214] = 50.0; f[1, 0, 0] = 50.0
    out["winner-at-the-last-element"] = (f, None)
    f = rng.standard_normal((3, 2, FL)); f[0, 1, 17] = np.inf; f[1, 0, 3] = f[1, 1, 3] = np.inf; f[2, 0, 0] = -np.inf
    out["plus-infinity"] = (f, None)
    f = rng.standard_normal((3, 2, FL)) * 1e-310; f[0, 0, 1] = 5e-324; f[0, 0, 2] = -5e-324; f[1] = np.abs(f[1]); f[2, 1] = 0.0
    out["denormals"] = (f, None)
    f = rng.standard_normal((3, 2, FL)); f[0, 0, ::2] = np.nan; f[1, 1, 5] = -np.nan; f[2, 0] = np.nan; f[2, 1, 1:] = np.nan
    f.view(np.uint64)[1, 0, 9] = 0xFFFFFFFFFFFFFFFF; f.view(np.uint64)[1, 0, 10] = 0x7FF0000000000001
    out["nan-inside-a-row"] = (f, None)
    f = rng.standard_normal((3, 1, FL)); f[0, 0, 5:] = -np.inf; f[1, 0, :] = -np.inf; f[1, 0, 1214] = 1.0
    out["fewer-candidates-than-entries"] = (f, None)
    return out
