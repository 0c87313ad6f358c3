"""tests/mutants.py is held to the sources and to the suite, on the CPU: every `old` text occurs exactly once in its file, every killer
is a test that exists, no id repeats, every translation unit that defines a kernel has at least two entries, and at most three entries
are declared equivalent.  A kernel edited so that a mutant no longer applies, or a killer renamed, fails here by naming the entry."""
import glob
import os
import re

import mutants as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "echoseal_amd", "csrc")
# es_scl_wide_large.hip compiles es_scl_wide.hip's kernel for two more capacities: it counts with that file
COUNTS_WITH = {"es_scl_wide_large.hip": "es_scl_wide.hip"}


def includes(name, seen=None):
    """The files under csrc that `name` includes, directly or not, itself included."""
    seen = set() if seen is None else seen
    if name in seen or not os.path.exists(os.path.join(CSRC, name)):
        return seen
    seen.add(name)
    for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(os.path.join(CSRC, name)).read(), re.M):
        includes(os.path.basename(inc), seen)
    return seen


def kernel_units():
    """{translation unit: the files it is compiled from} for every .hip file whose text, includes and all, defines a __global__ kernel."""
    units = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip"))):
        name = os.path.basename(path)
        files = includes(name)
        if any(re.search(r"^\s*(?:template\s*<[^>]*>\s*)?__global__", open(os.path.join(CSRC, f)).read(), re.M) for f in files):
            units[name] = files
    return units


def problems(mutants, read=lambda f: open(os.path.join(CSRC, f)).read(), test_exists=None):
    """What is wrong with a table, one line per finding, each naming its entry."""
    out = []
    seen = set()
    for m in mutants:
        if not re.fullmatch(r"[a-z0-9_]+", m.id):
            out.append(f"{m.id}: id is not [a-z0-9_]+")
        if m.id in seen:
            out.append(f"{m.id}: id repeats")
        seen.add(m.id)
        try:
            count = read(m.file).count(m.old)
        except OSError:
            count = -1
        if count != 1:
            out.append(f"{m.id}: `old` occurs {count} times in {m.file}, not once")
        if m.old == m.new:
            out.append(f"{m.id}: `new` equals `old`")
        if not isinstance(m.killers, tuple) or not m.killers:
            out.append(f"{m.id}: no killers")
        else:
            for k in m.killers:
                if not (test_exists or killer_exists)(k):
                    out.append(f"{m.id}: killer {k} does not exist")
        if len(m.why.split()) < 8 or not m.why.rstrip().endswith((".", ".)")):
            out.append(f"{m.id}: no sentence on why the change is value-only")
        if m.equivalent is not None and len(m.equivalent.split()) < 12:
            out.append(f"{m.id}: declared equivalent without an argument")
    if sum(m.equivalent is not None for m in mutants) > 3:
        out.append("more than three entries are declared equivalent: " + ", ".join(m.id for m in mutants if m.equivalent is not None))
    return out


def killer_exists(node):
    """tests/<file>.py::<test>: the file exists, defines the test and is a GPU test."""
    m = re.fullmatch(r"(tests/test_\w+\.py)::(test_\w+)", node)
    if not m or not os.path.exists(os.path.join(ROOT, m.group(1))):
        return False
    text = open(os.path.join(ROOT, m.group(1))).read()
    return bool(re.search(r"^def " + re.escape(m.group(2)) + r"\(", text, re.M)) and bool(re.search(r"^(pytestmark = |@)pytest\.mark\.gpu", text, re.M))


def unit_counts(mutants, units):
    counts = {}
    for unit, files in units.items():
        counts.setdefault(COUNTS_WITH.get(unit, unit), 0)
        if unit not in COUNTS_WITH:
            counts[unit] += sum(m.file in files for m in mutants)
    return counts


def test_the_table_fits_the_sources_and_the_suite():
    assert len(M.MUTANTS) >= 40
    found = problems(M.MUTANTS)
    assert not found, "\n".join(found)


def test_every_kernel_file_has_two_entries():
    units = kernel_units()
    assert len(units) >= 14 and "es_api.hip" not in units and {"es_sync.hip", "es_mix.hip", "es_scl_wide_large.hip"} <= set(units)
    thin = {u: n for u, n in unit_counts(M.MUTANTS, units).items() if n < 2}
    assert not thin, f"translation units with kernels and fewer than two entries in tests/mutants.py: {thin}"
    # the list decoders compile slowly: at most four entries are written in their files or compiled into all of them
    slow = [m.id for m in M.MUTANTS if m.file.startswith("es_scl") or all(m.file in units[u] for u in ("es_scl.hip", "es_scl_multi.hip", "es_scl_wide.hip"))]
    assert len(slow) <= 4, slow


def test_the_check_names_what_it_finds():
    """The checks above on small tables with one fault each: the finding names the entry."""
    good = M.Mutant("a_b1", "x.hip", "a > b", "a >= b", ("tests/test_gpu_x.py::test_y",), "A comparison inside a value computation, stored only.")
    read = lambda f: "if (a > b) c = a;"                                        # noqa: E731
    exists = lambda k: k == "tests/test_gpu_x.py::test_y"                        # noqa: E731
    assert problems([good], read, exists) == []
    assert "occurs 0 times" in problems([good._replace(old="a < b")], read, exists)[0]
    assert "occurs 2 times" in problems([good], lambda f: "a > b; a > b;", exists)[0]
    assert "killer tests/test_gpu_x.py::test_z does not exist" in problems([good._replace(killers=("tests/test_gpu_x.py::test_z",))], read, exists)[0]
    assert problems([good, good], read, exists) == ["a_b1: id repeats"]
    assert "id is not" in problems([good._replace(id="A-b")], read, exists)[0]
    four = [good._replace(id=f"e{i}", equivalent="no input can tell the two forms apart because the operand is never zero or a NaN") for i in range(4)]
    assert "more than three" in problems(four, read, exists)[-1]
    units = {"x.hip": {"x.hip", "x_body.inc"}, "y.hip": {"y.hip"}}
    assert unit_counts([good, good._replace(id="c", file="x_body.inc")], units) == {"x.hip": 2, "y.hip": 0}
    assert killer_exists("tests/test_gpu_memo.py::test_zero_records_write_nothing")
    assert not killer_exists("tests/test_gpu_memo.py::test_no_such_test") and not killer_exists("tests/test_grid_caps_listed.py::test_launch_sizes_and_index_sets")



def test_the_saturation_margin_cannot_move_a_threshold():
    """Why `MARG = 2.5 * DELTA -> 1.5 * DELTA` (sync_pick_row's saturation shortcut, es_sync32.hip) is not in the table: the shortcut sets
    thr = 0.95 when lo(bl) - MARG + K (j / 128 - MARG) >= 0.95 + 1e-6, K = 4.5 * 1.4826, for the median's bin bl in 1 .. 254 and a count j
    in 0 .. 63 of bins; the same histogram proves med >= lo(bl) - DELTA and MAD >= j / 128 - 2 DELTA (a screen value is within DELTA of
    the exact one, and the float32 bin index is off by less than 2e-7), so thr >= lo(bl) - DELTA + K (j / 128 - 2 DELTA) whatever the
    row.  A smaller margin is wrong only for a pair (bl, j) where the first holds and that bound is below 0.95: there is none for any
    margin from 2.5 * DELTA down to 0, so the outputs thr, peaks and npeaks cannot change.  The constants are read from the source."""
    src = open(os.path.join(CSRC, "es_sync32.hip")).read()
    delta = float(re.search(r"constexpr double DELTA = ([0-9.e-]+);", src).group(1))
    marg = float(re.search(r"constexpr double MARG = ([0-9.]+) \* DELTA;", src).group(1))
    assert "constexpr double BINW = 1.0 / 128.0;" in src and "(int)((v + 1.0f) * 128.0f)" in src
    sat = "const bool sat = bl >= 1 && bh <= 254 && jmax >= 0 && mL + (4.5 * 1.4826) * (jmax * BINW - MARG) >= 0.95 + 1e-6;"
    assert sat in src and "const double mL = (-1.0 + bl * BINW) - MARG;" in src and "const int j = lane;" in src
    k, eps = 4.5 * 1.4826, 2e-7
    assert (delta, marg) == (3e-5, 2.5)

    def wrong(m):
        return [(bl, j) for bl in range(1, 255) for j in range(64)
                if (-1.0 + bl / 128 - m * delta) + k * (j / 128 - m * delta) >= 0.95 + 1e-6
                and (-1.0 + bl / 128 - delta - eps) + k * (j / 128 - 2 * delta - 2 * eps) < 0.95]
    for m in (2.5, 2.0, 1.5, 1.0, 0.5, 0.0):
        assert wrong(m) == [], m
    assert wrong(-30.0)                                                      # the enumeration can find one: a large margin of the wrong sign


# ---------------------------------------------------------------------------------------------------------------- the list decoders
SCL_FILES = ("es_scl.hip", "es_scl_multi.hip", "es_scl_wide.hip", "es_math.h", "es_softplus_dev.h")
# what computes or is a subscript, a slab, LDS or slot address, a trip count or a barrier in the list decoders: no entry's text may name one
SCL_INDEX_NAMES = ("p8_get", "p8_set", "ptr_get", "ptr_set", "fp0", "myr", "holder", "parent", "src", "W.sel", "TBW", "TBA", "CB[", "cnt", "keep",
                   "nc", "info_idx +", "++info_idx", "dirty", "group_sync", "__syncthreads", "wave_fence", "ki & 127", "ES_EXP_TAB_LDS_ADDR",
                   "dpp", "swizzle", "bpermute", "asm", "<<<", "atomic", "slot", "cursor")


def asm_spans(text):
    """[start, end) of every `asm(` ... `)` or `asm volatile(` ... `)` block of a source text, parentheses balanced."""
    spans = []
    for m in re.finditer(r"\basm\s*(?:volatile\s*)?\(", text):
        depth, i = 1, m.end()
        while depth and i < len(text):
            depth += {"(": 1, ")": -1}.get(text[i], 0)
            i += 1
        spans.append((m.start(), i))
    return spans


def names_an_index(text, names=SCL_INDEX_NAMES):
    """The index helpers, counts and barriers that a mutant's text names; a plain word counts only as a whole identifier."""
    return [n for n in names if (re.search(r"(?<![A-Za-z0-9_])" + re.escape(n) + r"(?![A-Za-z0-9_])", text) if re.fullmatch(r"\w+", n) else n in text)]


def test_the_list_decoder_table_fits_the_sources_and_the_suite():
    found = problems(M.SCL_MUTANTS)
    assert not found, "\n".join(found)
    assert not {m.id for m in M.SCL_MUTANTS} & {m.id for m in M.MUTANTS}
    assert len(M.BY_ID) == len(M.MUTANTS) + len(M.SCL_MUTANTS) and all(M.BY_ID[m.id] is m for m in M.MUTANTS + M.SCL_MUTANTS)


def test_the_list_decoder_table_covers_every_file():
    assert 28 <= len(M.SCL_MUTANTS) <= 40
    per_file = {f: sum(m.file == f for m in M.SCL_MUTANTS) for f in SCL_FILES}
    assert all(n >= 4 for n in per_file.values()), per_file
    assert sum(per_file.values()) == len(M.SCL_MUTANTS), sorted({m.file for m in M.SCL_MUTANTS} - set(SCL_FILES))
    equivalent = [m.id for m in M.SCL_MUTANTS if m.equivalent is not None]
    assert len(equivalent) <= 4, equivalent


def test_no_list_decoder_entry_touches_an_asm_block_or_an_index():
    for m in M.SCL_MUTANTS:
        text = open(os.path.join(CSRC, m.file)).read()
        at = text.index(m.old)
        inside = [s for s in asm_spans(text) if s[0] < at + len(m.old) and at < s[1]]
        assert not inside, f"{m.id}: `old` lies inside an asm block"
        assert not asm_spans(m.new) and "asm" not in m.new, f"{m.id}: `new` holds an asm block"
        named = names_an_index(m.old) + names_an_index(m.new)
        assert not named, f"{m.id}: names {named}"
    # the two checks find what they look for
    src = 'x = a; asm volatile("v_mov_b64 %0, %1" : "=v"(x) : "s"(K)); y = b;'
    (lo, hi), = asm_spans(src)
    assert src[lo:hi].startswith("asm volatile(") and src[hi:] == "; y = b;"
    assert names_an_index("W.sel[fp0 + rank] = c") == ["fp0", "W.sel"] and names_an_index("rank < keep") == ["keep"]
    assert names_an_index("(mk == mc && k < cc_)") == [] and names_an_index("nc_") == [] and names_an_index("const int nc = 2 * cnt;") == ["cnt", "nc"]


def test_no_code_has_a_frozen_even_leaf_before_an_information_leaf():
    """Why `lp_odd = sp_sum` -> `sp_diff` in the frozen arm of es_scl.hip and es_scl_multi.hip is declared equivalent: the line's value is
    read only after a frozen even leaf that is decided leaf by leaf, which is leaf 0 or an even leaf whose odd sibling carries information
    (any other frozen even leaf opens a rate-0 block).  The oracle's frozen sets, which tests/test_oracle_polar.py pins to the reference
    and the device tables are compared with, have neither for any K the engine accepts."""
    from oracle import oracle as O
    O.build()
    for K in range(9, 1025):
        with O.code_k(K):
            frozen, _ = O.polar_tables()
        assert int(frozen.sum()) == 1024 - K and not frozen[0], K
        assert not (frozen[0::2] & ~frozen[1::2]).any(), K
    for name in ("es_scl.hip", "es_scl_multi.hip"):                          # the block arm is taken at every even leaf but leaf 0
        text = open(os.path.join(CSRC, name)).read()
        assert re.search(r"if \(\(i & 1\) == 0 && (P >= 2 && )?i != 0\) \{", text), name
    assert "launch_scl<64>" not in open(os.path.join(CSRC, "es_scl.hip")).read()       # P = 64 / L >= 2 in es_scl.hip
