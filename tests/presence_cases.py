"""The clips of the presence tests, shared by tests/test_presence_host.py and tests/test_gpu_presence.py: white-noise hosts
marked by the host WatermarkEmbedder in 1024-sample blocks with reproducible payloads, the first 777 samples cut off, so that the first
whole frame carries counter 1 and starts at sample 1215 - 777 = 438; and their four correlation rows from the CPU oracle."""
import functools

import numpy as np

from echoseal_amd.embedder import WatermarkEmbedder, synthetic_payloads
from echoseal_amd.tables import pack_tables

KEY = bytes(range(1, 33))
OTHER_KEY = b"\x5C" * 32
CUT = 777
FOUND = (1, 1215 - CUT)                                  # (counter, phase) of the first whole frame
SPAN = (0, 64)
# name -> (host sigma, seconds at 48 kHz, seed of the marked clip's host and payloads, seed of the unmarked host): A and B of DESIGN 4.23's
# table (B is seed 5).  A negative case is a 1-in-33 event by construction; B's own host is one (0.1647 against a decoy maximum of
# 0.1621), so B's unmarked case is the host of seed 6: the seed was changed, not the rule.
CLIPS = {"A": (0.005, 2.0, 3, 3), "B": (0.02, 2.0, 5, 6)}


def host(name: str, seconds: float | None = None, unmarked: bool = False) -> np.ndarray:
    sigma, secs, seed = CLIPS[name][0], CLIPS[name][1], CLIPS[name][3 if unmarked else 2]
    n = int(round((seconds or secs) * 48_000))
    return (sigma * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def marked(name: str, key: bytes = KEY, seconds: float | None = None) -> np.ndarray:
    """The host of `name` marked from counter 0 in 1024-sample blocks, without its first 777 samples."""
    x = host(name, seconds)
    emb = WatermarkEmbedder(key)
    payloads = synthetic_payloads(emb.sec, range(x.size // 1215 + 2), seed=CLIPS[name][2])
    emb._build_payload = lambda: payloads[emb.frame_ctr]                    # reproducible: process() draws its payloads from the system otherwise
    out = np.concatenate([emb.process(x[i:i + 1024]) for i in range(0, x.size, 1024)]).astype(np.float32)
    return out[CUT:]


def unmarked(name: str) -> np.ndarray:
    return host(name, unmarked=True)[CUT:]


def oracle_rows(O, clip: np.ndarray):
    """-> (corr float64 [4, n - 62] in BAND_PLAN order, nlag): oracle.lfilter and oracle.ncc with the engine's own tables."""
    ba, tpl, _, _, _ = pack_tables()
    x = np.ascontiguousarray(clip, np.float32)
    return np.stack([O.ncc(O.lfilter(ba[b, :9], ba[b, 9:], x), tpl[b, :63]) for b in range(4)]), x.size - 62


@functools.lru_cache(maxsize=None)
def cached(kind: str, name: str) -> np.ndarray:
    """The clips by name, made once per session: kind in marked / unmarked."""
    clip = {"marked": lambda: marked(name), "unmarked": lambda: unmarked(name)}[kind]()
    clip.setflags(write=False)
    return clip
