"""Every launcher that caps its grid (es_grid in echoseal_amd/csrc/*.hip) is listed in tests/grid_caps.py with the test that drives it
past its cap or a written reason why none can: a new capped launcher without either fails here, on the CPU."""
import glob
import os
import re

import grid_caps as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "echoseal_amd", "csrc")


def capped_launchers():
    """{es_launch_* function: [file:line of each es_grid( call inside it]} over the .hip sources."""
    found = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip"))):
        current = None
        for no, line in enumerate(open(path), 1):
            m = re.match(r"^(?:static\s+)?int\s+(es_launch_\w+)\s*\(", line)
            if m:
                current = m.group(1)
            if "es_grid(" in line:
                assert current is not None, f"{os.path.basename(path)}:{no}: es_grid( outside an es_launch_* function"
                found.setdefault(current, []).append(f"{os.path.basename(path)}:{no}")
    return found


def test_every_capped_launcher_is_listed():
    found = capped_launchers()
    assert len(found) >= 30                                                    # the scan still finds them
    missing = {name: at for name, at in found.items() if name not in G.LAUNCHERS}
    assert not missing, f"capped launchers without a past-the-cap test or an exemption in tests/grid_caps.py: {missing}"
    stale = sorted(set(G.LAUNCHERS) - set(found))
    assert not stale, f"tests/grid_caps.py lists launchers that no longer call es_grid: {stale}"


def test_every_entry_names_an_existing_test_or_gives_a_reason():
    for name, entry in G.LAUNCHERS.items():
        if isinstance(entry, G.Exempt):
            assert len(entry.why.split()) >= 8 and entry.why.rstrip().endswith("."), name
            continue
        assert isinstance(entry, G.Driven), name
        path = os.path.join(ROOT, "tests", entry.file)
        assert os.path.exists(path), (name, entry.file)
        assert re.search(r"^def " + re.escape(entry.test) + r"\(", open(path).read(), re.M), (name, entry.file, entry.test)


def test_launch_sizes_and_index_sets():
    for cap in (16 * 256, 64 * 256, 8 * 256 * 256, 2048 * 304):
        n = G.past(cap)
        assert cap < n < 2 * cap and all(n % b for b in (4, 64, 256, 1024))
    idx = G.index_set(100, [30, 45], seed=1)
    assert {0, 29, 30, 31, 44, 45, 46, 59, 60, 61, 89, 90, 91, 99} <= set(idx.tolist()) and idx.max() == 99 and len(idx) <= 14 + 6 + 16
    assert [(s.start, s.stop) for s in G.slices(10, 4)] == [(0, 4), (4, 8), (8, 10)]
