"""CPU: the crafted AEAD edge vectors of tests/aead_edges.py are what they claim to be.  Their Poly1305 accumulators land on
chosen residues mod 2^130 - 5; the branch-taking ones take the final conditional subtraction of the 26-bit limb code
(es_aead.hip's Poly::finish, oracle/c/eso_aead.c); dropping that subtraction changes their tags.  The C oracle and the
big-integer host primitives agree on all of them.  tests/test_gpu_aead_edges.py runs the same vectors through the HIP kernels."""
import numpy as np
import pytest

from aead_edges import BRANCH_RESIDUES, KEYS, RESIDUES, crafted_vectors, mac_input, poly1305_limbs
from echoseal_amd.primitives import poly1305_tag


@pytest.fixture(scope="module")
def oracle():
    import oracle.oracle as o
    o.build()
    return o


@pytest.fixture(scope="module")
def vectors():
    return {name: crafted_vectors(key) for name, key in KEYS.items()}


def test_crafted_vectors_reach_the_final_subtraction(vectors):
    branch = 0
    wraps = set()
    for name, vs in vectors.items():
        assert sorted({v.residue for v in vs}) == sorted(RESIDUES), name
        for v in vs:
            msg = mac_input(v.ct)
            tag, took = poly1305_limbs(v.otk, msg)
            assert tag == v.tag == poly1305_tag(v.otk, msg), (name, v.residue)
            assert took == (v.residue in BRANCH_RESIDUES), (name, v.residue)
            assert v.plain[:4] == b"ESAL"
            branch += took
            wraps.add(v.wraps)
    assert branch >= 20
    assert wraps == {False, True}          # (h mod p) + s carries past 2^128 for some vectors and not for others


def test_vectors_catch_a_missing_final_subtraction(vectors):
    for name, vs in vectors.items():
        for v in vs:
            msg = mac_input(v.ct)
            bad, _ = poly1305_limbs(v.otk, msg, final_subtract=False)
            assert (bad != v.tag) == v.branch, (name, v.residue)


def test_oracle_accepts_crafted_vectors(oracle, vectors):
    for name, vs in vectors.items():
        key = KEYS[name]
        blobs = np.stack([np.frombuffer(v.blob, np.uint8) for v in vs])
        ctrs = np.array([v.ctr for v in vs], np.uint32)
        ok, plain = oracle.validate_blobs(key, blobs, ctrs)
        assert ok.all(), name
        assert [p.tobytes() for p in plain] == [v.plain for v in vs], name
        # one flipped tag bit: rejected, plaintext withheld
        i = np.arange(len(vs))
        bad = blobs.copy(); bad[i, 39 + i % 16] ^= (1 << (i % 8)).astype(np.uint8)
        ok, plain = oracle.validate_blobs(key, bad, ctrs)
        assert not ok.any() and not plain.any(), name
        for v in vs:
            msg = mac_input(v.ct)
            assert oracle.poly1305(v.otk, msg) == poly1305_tag(v.otk, msg) == v.tag, (name, v.residue)


@pytest.mark.parametrize("otk", [bytes(range(1, 33)), b"\x00" * 32, b"\xFF" * 32, b"\xAA" * 32])
def test_poly1305_partial_blocks(oracle, otk):
    """Lengths 0..80 of all-0x00 and all-0xFF messages: every short last block, the zero-length message."""
    for fill in (0x00, 0xFF):
        for n in range(81):
            msg = bytes([fill]) * n
            want = poly1305_tag(otk, msg)
            assert oracle.poly1305(otk, msg) == want, (fill, n)
            assert poly1305_limbs(otk, msg)[0] == want, (fill, n)
