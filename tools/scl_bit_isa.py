"""Vector instructions of the per-bit path of the headline list decoder (es_scl_wide_kernel<64, 8, false>), read from its gfx950 assembly
without a GPU: the basic blocks that hold the sort network's compare-exchange steps -- an unfrozen leaf's decision, sort, survivor gather and
the start of the partial-sum fold are one straight block (two since the even and the odd leaf are separate code) -- and the blocks that
evaluate a leaf's own softplus.
    python3 tools/scl_bit_isa.py [--asm FILE.s] [--label NAME --into FILE.json]
Columns: vector = every v_* instruction, steps = compare-exchange steps (borrow chains / 2 per element pair), swizzle / bpermute = the
cross-lane fetches that go through the LDS crossbar, shifts_64bit = v_lshl / lshr / ashr of 64 bits in the whole kernel."""
import argparse, json, os, re, sys, tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from scl_f_isa import HEADLINE, ROOT, build_asm, kernel_lines  # noqa: E402


def all_blocks(lines):
    cur, res = None, []
    for line in lines:
        s = line.strip()
        m = re.match(r"^(\.LBB\d+_\d+):", s) or re.match(r"^; %bb\.(\d+):", s)
        if m:
            cur = {"label": m.group(1), "ins": []}
            res.append(cur)
            continue
        if cur is None or not s or s.startswith(";") or s.startswith("."):
            continue
        cur["ins"].append(s.split()[0])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--csrc", default=os.path.join(ROOT, "echoseal_amd", "csrc"))
    ap.add_argument("--asm")
    ap.add_argument("--label")
    ap.add_argument("--into")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        path = a.asm
        if path is None:
            path = os.path.join(tmp, "es_scl_wide.s")
            build_asm(os.path.abspath(a.csrc), path)
        bl = all_blocks(kernel_lines(path, HEADLINE))
    n = lambda b, pre: sum(op.startswith(pre) for op in b["ins"])
    rows = []
    for b in bl:
        steps = n(b, "v_subb_co_u32") // 2
        if steps:
            rows.append({"block": b["label"], "vector": n(b, "v_"), "instructions": len(b["ins"]), "steps": steps,
                         "swizzle": n(b, "ds_swizzle"), "bpermute": n(b, "ds_bpermute"), "lane_moves": n(b, "v_readlane") + n(b, "v_writelane")})
    res = {"kernel": HEADLINE, "sort_blocks": rows, "vector_per_unfrozen_leaf": round(sum(r["vector"] for r in rows) / max(1, len(rows)), 1),
           "shifts_64bit": sum(1 for b in bl for op in b["ins"] if re.match(r"v_(lshl|lshr|ashr)rev_[bi]64", op)),
           "static_vector": sum(n(b, "v_") for b in bl), "static_instructions": sum(len(b["ins"]) for b in bl)}
    print(f"{'block':>12} {'vector':>7} {'all':>5} {'steps':>6} {'swizzle':>8} {'bpermute':>9} {'lane_moves':>11}")
    for r in rows:
        print(f"{r['block']:>12} {r['vector']:>7} {r['instructions']:>5} {r['steps']:>6} {r['swizzle']:>8} {r['bpermute']:>9} {r['lane_moves']:>11}")
    print(json.dumps({k: v for k, v in res.items() if k != "sort_blocks"}))
    if a.into:
        doc = json.load(open(a.into)) if os.path.exists(a.into) else {}
        doc[a.label or "result"] = res
        with open(a.into, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
