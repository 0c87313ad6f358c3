#!/usr/bin/env python3
"""Mutant audit of the GPU suite: does a test fail when a constant, a comparison or a tie rule of a kernel is changed?

  tools/mutant_audit.py build [ids...]   no GPU: one library per entry of tests/mutants.py, echoseal_amd/libechoseal_hip_<id>.so
  tools/mutant_audit.py run [ids...]     on the GPU: each entry's killers against its library, results into profiles/mutants.json

Without ids both take a whole table: `--table dsp` (the default) is MUTANTS, `--table scl` SCL_MUTANTS, the list decoders.

build copies echoseal_amd/csrc to a scratch directory per entry, applies the entry's substitution there (it must apply exactly once),
compiles only the translation units that include the changed file, with the Makefile's flags and per-file flags, and links them with
the stock objects.  Compiles and links share one pool of 16 jobs.  No mutated source is kept.

run first measures, on the unmutated library, every distinct killer set of the chosen entries (record `baseline`), then runs for each
entry in turn, in a fresh child process,
    timeout -k 10 <limit> env ES_LIB_VARIANT=<id> python -m pytest -x -q -m gpu <killers>
with <limit> = three times the set's unmutated time, rounded up to 10 s.  Exit status 1 with a FAILED test = killed, 0 = survived; ANY
other status, a status 1 without a failed test (errors in fixtures or at collection are not kills), or `illegal memory access` /
`HSA_STATUS_ERROR` in the child's output, stops the whole run there: nothing further is started, the records
so far are in the file, and the run is continued (`--resume FILE`, with the remaining ids) only after the cause has been read from what
it left.  Nothing is ever tried twice.  After the last entry, a survivor that is not declared equivalent gets one more run against the
whole `-m gpu` suite, under the suite's own unmutated time (measured when the first survivor needs it) with the same margin;
`--suite-max N` gives that run to the first N such survivors only, in table order, and records the others "suite_status": "not run".
Before the first child starts, run refuses an entry whose library has not been built.
"""
import argparse
import concurrent.futures
import json
import math
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "echoseal_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mutants as M  # noqa: E402

JOBS = 16
FAULT_WORDS = ("illegal memory access", "HSA_STATUS_ERROR")
BASELINE_LIMIT = 600                       # the unmutated killers of one set; the whole suite gets SUITE_LIMIT
SUITE_LIMIT = 1100


TABLES = {"dsp": lambda: M.MUTANTS, "scl": lambda: M.SCL_MUTANTS}


def chosen(ids, table="dsp"):
    unknown = [i for i in ids if i not in M.BY_ID]
    if unknown:
        sys.exit(f"no such entry in tests/mutants.py: {unknown}")
    return [M.BY_ID[i] for i in ids] if ids else list(TABLES[table]())


# ---------------------------------------------------------------------------------------------------------------- build
def includes(name, seen=None):
    seen = set() if seen is None else seen
    if name in seen or not os.path.exists(os.path.join(CSRC, name)):
        return seen
    seen.add(name)
    for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(os.path.join(CSRC, name)).read(), re.M):
        includes(os.path.basename(inc), seen)
    return seen


def makefile():
    text = open(os.path.join(CSRC, "Makefile")).read()
    var = lambda name: re.search(r"^" + name + r"\s*[:?]?=\s*(.*)$", text, re.M).group(1).strip()      # noqa: E731
    arch = var("ARCH")
    flags = var("HIPFLAGS").replace("$(ARCH)", arch).split()
    per_file = {m.group(1): m.group(2).split() for m in re.finditer(r"^FLAGS_(\w+)\s*:=\s*(.*)$", text, re.M)}
    return var("HIPCC"), arch, flags, per_file, var("SRCS").split()


def build_one(m, pool, hipcc, arch, flags, per_file, srcs):
    """-> (id, seconds, units): scratch copy, substitution, compile the units that include m.file, link with the stock objects."""
    t0 = time.time()
    scratch = tempfile.mkdtemp(prefix=f"mutant_{m.id}_")
    try:
        csrc = os.path.join(scratch, "echoseal_amd", "csrc")
        shutil.copytree(CSRC, csrc, ignore=shutil.ignore_patterns("*.o", "*.so"))
        shutil.copytree(os.path.join(ROOT, "include"), os.path.join(scratch, "include"))
        path = os.path.join(csrc, m.file)
        text = open(path).read()
        if text.count(m.old) != 1:
            raise SystemExit(f"{m.id}: `old` occurs {text.count(m.old)} times in {m.file}, not once: nothing built")
        open(path, "w").write(text.replace(m.old, m.new))
        units = [s for s in srcs if m.file in includes(s)]
        if not units:
            raise SystemExit(f"{m.id}: no translation unit includes {m.file}")

        def compile_unit(unit):
            stem = unit[:-len(".hip")]
            cmd = [hipcc] + flags + per_file.get(stem, []) + ["-c", unit, "-o", stem + ".o"]
            r = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True)
            if r.returncode != 0:
                raise SystemExit(f"{m.id}: {unit} does not compile:\n{r.stderr[-2000:]}")
        list(pool.map(compile_unit, units))
        objs = [os.path.join(csrc, u[:-4] + ".o") if u in units else os.path.join(CSRC, u[:-4] + ".o") for u in srcs]
        out = os.path.join(ROOT, "echoseal_amd", f"libechoseal_hip_{m.id}.so")
        pool.submit(subprocess.run, [hipcc, "-shared", "-fPIC", f"--offload-arch={arch}", "-o", out] + objs, check=True).result()
        return m.id, round(time.time() - t0, 1), units
    finally:
        shutil.rmtree(scratch, ignore_errors=True)


def cmd_build(args):
    todo = chosen(args.ids, args.table)
    subprocess.run(["make", "-s", f"-j{JOBS}", "-C", CSRC], check=True)                      # the stock objects and library
    hipcc, arch, flags, per_file, srcs = makefile()
    # one pool of JOBS jobs for every compile and every link; an entry's driver thread copies the sources and waits for its jobs
    with concurrent.futures.ThreadPoolExecutor(JOBS) as pool, concurrent.futures.ThreadPoolExecutor(JOBS) as drivers:
        futures = [drivers.submit(build_one, m, pool, hipcc, arch, flags, per_file, srcs) for m in todo]
        for f in futures:
            mid, sec, units = f.result()
            print(f"built libechoseal_hip_{mid}.so  ({', '.join(units)}; {sec} s)", flush=True)
    print(f"{len(todo)} libraries built")


# ---------------------------------------------------------------------------------------------------------------- run
def limit_for(seconds):
    return int(math.ceil(3.0 * seconds / 10.0) * 10)


def child(limit, variant, targets):
    """One pytest child under its own time limit -> (exit status, seconds, first failing test, output)."""
    env = ["env", f"ES_LIB_VARIANT={variant}"] if variant else ["env", "-u", "ES_LIB_VARIANT"]
    cmd = ["timeout", "-k", "10", str(limit)] + env + [sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu"] + list(targets)
    t0 = time.time()
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, stdin=subprocess.DEVNULL)
    failed = re.search(r"^FAILED (.+?)(?: - .*)?$", r.stdout, re.M)            # the node id whole: a parameter may hold spaces
    return r.returncode, round(time.time() - t0, 1), failed.group(1) if failed else None, r.stdout


class Stop(Exception):
    pass


def cmd_run(args):
    todo = chosen(args.ids, args.table)
    records = []
    if args.resume:
        records = json.load(open(args.resume))
    base = next((r for r in records if r["id"] == "baseline"), None)
    if base is None:
        base = {"id": "baseline", "status": "passed", "seconds": 0.0, "sets": {}, "suite_seconds": None}
        records.insert(0, base)
    unbuilt = [m.id for m in todo if not os.path.exists(os.path.join(ROOT, "echoseal_amd", f"libechoseal_hip_{m.id}.so"))]
    if unbuilt:
        sys.exit(f"not built (tools/mutant_audit.py build): {unbuilt}; nothing was run")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def save():
        with open(args.out + ".tmp", "w") as f:
            json.dump(records, f, indent=1)
            f.write("\n")
        os.replace(args.out + ".tmp", args.out)

    def checked(what, status, out, ok, failed="-"):
        """Stop the whole run on a fault word, on a status outside `ok`, or on a status 1 that names no failed test."""
        word = next((w for w in FAULT_WORDS if w in out), None)
        if word or status not in ok or (status == 1 and failed is None):
            tail = "\n".join(out.splitlines()[-25:])
            raise Stop(f"{what}: exit status {status}" + (f", output holds `{word}`" if word else "") + f"; nothing further is started\n{tail}")

    try:
        for key in sorted({" ".join(m.killers) for m in todo}):
            if key in base["sets"]:
                continue
            status, sec, failed, out = child(BASELINE_LIMIT, None, key.split())
            if status != 0:
                base["status"] = f"failed: {failed or status}"
                save()
            checked(f"baseline of {key}", status, out, (0,))
            base["sets"][key] = sec
            base["seconds"] = round(sum(base["sets"].values()), 1)
            print(f"baseline {sec:6.1f} s  {key}", flush=True)
            save()
        done = {r["id"] for r in records}
        for m in todo:
            if m.id in done:
                continue
            limit = limit_for(base["sets"][" ".join(m.killers)])
            status, sec, failed, out = child(limit, m.id, m.killers)
            verdict = "killed" if status == 1 and failed else "survived" if status == 0 else f"stopped: exit status {status}"
            rec = {"id": m.id, "status": verdict, "first_failing_test": failed,
                   "seconds": sec, "limit": limit, "equivalent": m.equivalent is not None}
            records.append(rec)
            save()
            print(f"{rec['status']:9s} {sec:6.1f} s  {m.id}  {failed or ''}", flush=True)
            checked(m.id, status, out, (0, 1), failed)
        # survivors of their own killers, the declared equivalents apart: does any test of the whole suite notice them?
        suite_runs = 0
        for m in todo:
            rec = next(r for r in records if r["id"] == m.id)
            if rec["status"] != "survived" or rec["equivalent"]:
                continue
            suite_runs += 1                                                    # --suite-max counts survivors in table order, a resumed file's included
            if rec.get("suite_status", "not run") != "not run":
                continue
            if args.suite_max is not None and suite_runs > args.suite_max:
                rec["suite_status"] = "not run"
                save()
                continue
            if base["suite_seconds"] is None:
                s_status, s_sec, s_failed, s_out = child(SUITE_LIMIT, None, ["tests"])
                if s_status != 0:
                    base["status"] = f"failed: {s_failed or s_status}"
                    save()
                checked("baseline of the whole suite", s_status, s_out, (0,))
                base["suite_seconds"] = s_sec
                print(f"baseline {s_sec:6.1f} s  the whole -m gpu suite", flush=True)
                save()
            s_limit = limit_for(base["suite_seconds"])
            s_status, s_sec, s_failed, s_out = child(s_limit, m.id, ["tests"])
            s_verdict = "killed" if s_status == 1 and s_failed else "survived" if s_status == 0 else f"stopped: exit status {s_status}"
            rec.update(suite_status=s_verdict,
                       suite_first_failing_test=s_failed, suite_seconds=s_sec, suite_limit=s_limit)
            save()
            print(f"whole suite: {rec['suite_status']} {s_sec:6.1f} s  {m.id}  {s_failed or ''}", flush=True)
            checked(m.id + " under the whole suite", s_status, s_out, (0, 1), s_failed)
    except Stop as stop:
        print(f"STOPPED  {stop}", flush=True)
        return 3
    left = [r["id"] for r in records if r["id"] != "baseline" and r["status"] == "survived" and not r["equivalent"]]
    print(f"{sum(r.get('status') == 'killed' for r in records)} killed, survivors that are not declared equivalent: {left or 'none'}")
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    b = sub.add_parser("build")
    b.add_argument("ids", nargs="*")
    r = sub.add_parser("run")
    r.add_argument("ids", nargs="*")
    for p in (b, r):
        p.add_argument("--table", choices=sorted(TABLES), default="dsp",
                       help="the table taken when no ids are given: dsp = MUTANTS, scl = SCL_MUTANTS, the list decoders (DESIGN 2.3)")
    r.add_argument("--suite-max", type=int, default=None, metavar="N",
                   help="only the first N survivors that are not declared equivalent, in table order, get the whole-suite run; "
                        "the others are recorded \"suite_status\": \"not run\" (default: all of them)")
    r.add_argument("--out", default=os.path.join(ROOT, "profiles", "mutants.json"))
    r.add_argument("--resume", help="the file of a run that stopped or covered other ids: its records are kept, its baseline times reused")
    args = ap.parse_args()
    sys.exit(cmd_build(args) if args.cmd == "build" else cmd_run(args))


if __name__ == "__main__":
    main()
