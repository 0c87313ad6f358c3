"""Pin the C oracle's demodulator (eso_llr) and header decoder (eso_decode_header) against the reference at the payload-length edges:
tests/golden/front_edges.npz, captured by running the reference's own _llr and _decode_header (oracle/refshim/gen_golden_edges.py).

The GPU tests (tests/test_gpu_front_edges.py) hold the kernels to the oracle bit for bit at every payload length 1 .. 1 024; this holds
the oracle to the reference where the kernels' length branches are: payloads 1 .. 64 and a spread up to 1 024 in all four bands,
frame slices of 189 .. 200 samples for the header, and degenerate rows (silence, constant, spike, periodic, alternating, extreme
amplitudes, noise), at 48 000 Hz and at 211 790 Hz (576-tap filters, the large build at capacity).

Bars as in test_golden_r2.py: LLR within 1e-5; the chosen shift equal, or a near-tie (best and runner-up within 1e-5 relative);
header ok and value exact, score within 1e-4, chosen shift equal."""
import os

import numpy as np
import pytest

from echoseal_amd.crypto import SecureChannel
from echoseal_amd.tables import pack_tables

HERE = os.path.dirname(os.path.abspath(__file__))
KEY = b"\xAA" * 32


@pytest.fixture(scope="module")
def edges():
    return np.load(os.path.join(HERE, "golden", "front_edges.npz"))


def _frame(g, i):
    return g["samples"][g["offsets"][i]:g["offsets"][i + 1]].astype(np.float64)


def test_fixture_covers_the_edges(edges):
    g = edges
    for fs in (48_000, 211_790):
        m = g["fs"] == fs
        npl = g["flen"][m & (g["kind"] == 0)] - 191
        assert set(range(1, 65)) <= set(npl.tolist()) and npl.max() == 1024
        for b in range(4):                                              # every length in every band
            mb = m & (g["kind"] == 0) & (g["band"] == b)
            assert set(range(1, 65)) <= set((g["flen"][mb] - 191).tolist())
        assert set(range(189, 201)) <= set(g["flen"][m & (g["kind"] == 1)].tolist())
        assert int((m & (g["kind"] >= 2)).sum()) == len(g["degenerate_names"])


@pytest.mark.parametrize("fs", [48_000, 211_790])
def test_oracle_llr_matches_reference_at_edges(oracle, edges, fs):
    g = edges
    ba, tpl, taps, ntaps, _ = pack_tables(fs)
    sec = SecureChannel(KEY)
    checked, ties = 0, []
    for i in np.flatnonzero(g["fs"] == fs):
        b = int(g["band"][i]); ctr = int(g["ctr"][i])
        fr = _frame(g, i)
        pn = sec.pn_bits(ctr, 1215)
        h = taps[b, :ntaps[b]]
        for variant, pnb in ((0, pn[191:1215]), (1, pn[:1024])):
            want = g[f"llr{variant}"][i]
            llr, best_s, s0, s1 = oracle.llr(fr, pnb, h)
            if fr.size <= 191:                                          # no payload: zeros, no shift search
                assert not llr.any() and not want.any() and best_s == 0, (i, variant)
                continue
            checked += 1
            if best_s != int(g["best_s"][i, variant]):
                margin = (s0 - s1) / max(abs(s0), 1e-30)
                assert margin < 1e-5, (i, variant, fr.size, best_s, int(g["best_s"][i, variant]), margin)
                ties.append((int(i), variant))
                continue
            err = float(np.max(np.abs(llr.astype(np.float64) - want)))
            assert err <= 1e-5, (i, variant, fr.size, err)
    assert checked >= 2 * 4 * (64 + 13) and len(ties) <= 2, (checked, ties)     # every length in every band, both variants


@pytest.mark.parametrize("fs", [48_000, 211_790])
def test_oracle_header_matches_reference_at_edges(oracle, edges, fs):
    g = edges
    ba, tpl, taps, ntaps, _ = pack_tables(fs)
    hdr_pn = SecureChannel(KEY).pn_bits(0, 128)
    n_full = 0
    for i in np.flatnonzero(g["fs"] == fs):
        b = int(g["band"][i])
        fr = _frame(g, i)
        ok, val, score, best_s = oracle.decode_header(fr, hdr_pn, taps[b, :ntaps[b]])
        w_ok, w_val, w_score, w_s = g["hdr"][i]
        assert ok == bool(w_ok) and val == int(w_val), (i, fr.size)
        assert abs(score - w_score) <= 1e-4 * max(1.0, abs(w_score)), (i, fr.size, score, w_score)
        assert best_s == int(w_s), (i, fr.size, best_s, int(w_s))
        n_full += fr.size >= 191
    assert n_full > 0
