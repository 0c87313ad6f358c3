"""Hot vector instructions per f evaluation of the headline list decoder (es_scl_wide_kernel<64, 8, false>), read from its gfx950
assembly without a GPU.
    python3 tools/scl_f_isa.py [--csrc DIR] [--asm FILE.s] [--label NAME --into FILE.json]
Builds the device assembly of es_scl_wide.hip with the Makefile's flags (or reads --asm), cuts the headline kernel into basic blocks
(a label or a fall-through comment opens one, the first branch closes its counted part: in an f loop that is the branch round the
out-of-range softplus) and prints, for every block that holds a v_rcp_f64 (each softplus has two), its vector instructions:
    vector  every v_* instruction            f64   v_add/mul/fma/fmac/max_f64            rcp   v_rcp_f64
    other   vector - f64 - rcp: selects, compares, table index and scale bits, moves, conversions, address arithmetic
    f       evaluations of f in the block (rcp / 4) or, where a block holds one softplus of an f, 0.5
A block that starts an f also holds what feeds it (loads' conversions, g, addresses), so compare like with like between two builds:
the blocks come out in the kernel's order, which a change to f does not alter.  --into merges the result under --label into a JSON
file (profiles/r07_scl_f_isa.json holds the parent's and the result's)."""
import argparse, json, os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = "_ZN12_GLOBAL__N_118es_scl_wide_kernelILi64ELi8ELb0EEEvNS_8WideArgsE"
F64 = re.compile(r"^v_(add|mul|fma|fmac|max)_f64")


def build_asm(csrc, out):
    mk = open(os.path.join(csrc, "Makefile")).read()
    hipcc = os.environ.get("HIPCC", re.search(r"^HIPCC\s*\?=\s*(\S+)", mk, re.M).group(1))
    flags = re.search(r"^HIPFLAGS\s*\?=\s*(.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").split()
    subprocess.check_call([hipcc, *flags, "-Wno-unused-command-line-argument", "--cuda-device-only", "-S", "es_scl_wide.hip", "-o", out], cwd=csrc)


def kernel_lines(path, name):
    on, out = False, []
    for line in open(path):
        if line.startswith(name + ":"):
            on = True
        elif on and ".end_amdhsa_kernel" in line:
            break
        if on:
            out.append(line.rstrip("\n"))
    if not out:
        sys.exit(f"{name} not found in {path}")
    return out


def blocks(lines):
    """(label, loop depth, instructions up to and including the first branch) of every basic block"""
    cur, res = None, []
    for line in lines:
        s = line.strip()
        m = re.match(r"^(\.LBB\d+_\d+):", s) or re.match(r"^; %bb\.(\d+):", s)
        if m:
            cur = {"label": m.group(1), "depth": None, "ins": [], "closed": False}
            d = re.search(r"Depth=(\d+)", s)
            if d:
                cur["depth"] = int(d.group(1))
            res.append(cur)
            continue
        if cur is None or not s or s.startswith(";") or s.startswith("."):
            continue
        op = s.split()[0]
        if cur["closed"]:
            continue
        cur["ins"].append(op)
        if op.startswith("s_cbranch") or op.startswith("s_branch") or op.startswith("s_swappc") or op.startswith("s_endpgm"):
            cur["closed"] = True
    return res


def count(lines):
    out = []
    for b in blocks(lines):
        rcp = sum(op.startswith("v_rcp_f64") for op in b["ins"])
        if not rcp:
            continue
        vec = sum(op.startswith("v_") for op in b["ins"])
        f64 = sum(bool(F64.match(op)) for op in b["ins"])
        out.append({"block": b["label"], "f": rcp / 4, "vector": vec, "f64": f64, "rcp": rcp, "other": vec - f64 - rcp,
                    "scratch": sum(op.startswith("scratch_") for op in b["ins"])})
    return out


def metadata(path, name):
    txt = open(path).read()
    i = txt.find(f".name:           {name}")
    j, k = txt.rfind("  - .agpr_count", 0, i), txt.find("  - .agpr_count", i)
    md = txt[j:k if k > 0 else len(txt)]
    return {key: int(re.search(rf"\.{key}:\s+(\d+)", md).group(1)) for key in ("vgpr_count", "vgpr_spill_count", "sgpr_count", "sgpr_spill_count")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--csrc", default=os.path.join(ROOT, "echoseal_amd", "csrc"))
    ap.add_argument("--asm")
    ap.add_argument("--kernel", default=HEADLINE)
    ap.add_argument("--label")
    ap.add_argument("--into")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        path = a.asm
        if path is None:
            path = os.path.join(tmp, "es_scl_wide.s")
            build_asm(os.path.abspath(a.csrc), path)
        lines = kernel_lines(path, a.kernel)
        rows = count(lines)
        res = {"kernel": a.kernel, **metadata(path, a.kernel),
               "scratch_in_f_blocks": sum(r["scratch"] for r in rows),
               "f_evaluations": sum(r["f"] for r in rows),
               "vector": sum(r["vector"] for r in rows), "f64": sum(r["f64"] for r in rows), "rcp": sum(r["rcp"] for r in rows),
               "other": sum(r["other"] for r in rows), "blocks": rows}
        res["other_per_f"] = round(res["other"] / res["f_evaluations"], 2)
    print(f"{'block':>12} {'f':>5} {'vector':>7} {'f64':>5} {'rcp':>4} {'other':>6} {'scratch':>8}")
    for r in rows:
        print(f"{r['block']:>12} {r['f']:>5} {r['vector']:>7} {r['f64']:>5} {r['rcp']:>4} {r['other']:>6} {r['scratch']:>8}")
    print(json.dumps({k: v for k, v in res.items() if k != "blocks"}))
    if a.into:
        doc = json.load(open(a.into)) if os.path.exists(a.into) else {}
        doc[a.label or "result"] = res
        with open(a.into, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
