#!/usr/bin/env python3
"""Do two builds of the library hold the same instructions?  For every object of pypbr_amd/csrc in each tree, every gfx950 function's
disassembly (mnemonics and operands, tools/check_isa.py's reader) is hashed; the report lists per object the number of kernels, whether
all of them are identical in both trees, and which symbols exist in one tree only.  No GPU needed.  What a pull request that adds a
translation unit records to show that no existing kernel changed:

    python tools/isa_digests.py --revs par=PATH_TO_PARENT_CHECKOUT,head=. --out profiles/ab_NAME_digests.json"""
import argparse
import hashlib
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_isa  # noqa: E402


def digests(tree):
    csrc = os.path.join(os.path.abspath(tree), "pypbr_amd", "csrc")
    out = {}
    for name in sorted(f for f in os.listdir(csrc) if f.endswith(".o") and f != "build_id.o"):
        with tempfile.TemporaryDirectory(prefix="pbr_isa_") as tmp:
            fns = check_isa._functions(check_isa._code_object(os.path.join(csrc, name), tmp))
        out[name] = {sym: hashlib.sha256("\n".join("%s %s" % i for i in insts).encode()).hexdigest()[:16] for sym, insts in fns.items()}
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--revs", required=True, help="alias=path,alias=path")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    (a, pa), (b, pb) = (r.split("=", 1) for r in args.revs.split(","))
    da, db = digests(pa), digests(pb)
    objects, all_same = [], True
    for name in sorted(set(da) | set(db)):
        fa, fb = da.get(name, {}), db.get(name, {})
        common = sorted(set(fa) & set(fb))
        differ = [s for s in common if fa[s] != fb[s]]
        rec = {"object": name, a: len(fa), b: len(fb), "identical": len(common) - len(differ), "differ": differ,
               "only_in_" + a: sorted(set(fa) - set(fb)), "only_in_" + b: sorted(set(fb) - set(fa)),
               "sha256_16_of_all": hashlib.sha256("".join(fb[s] for s in sorted(fb)).encode()).hexdigest()[:16]}
        all_same = all_same and not differ and not rec["only_in_" + a] and (name not in da or not rec["only_in_" + b])
        objects.append(rec)
    report = {"tool": "tools/isa_digests.py", "what": "per-function digests of the gfx950 disassembly of every object of pypbr_amd/csrc, two builds",
              "revisions": [a, b], "functions": {a: sum(len(v) for v in da.values()), b: sum(len(v) for v in db.values())},
              "objects_only_in_" + b: sorted(set(db) - set(da)), "every_function_of_" + a + "_is_identical_in_" + b: all_same, "objects": objects}
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
    print("%s: %d functions, %s: %d; every function of %s identical in %s: %s; new objects: %s"
          % (a, report["functions"][a], b, report["functions"][b], a, b, all_same, report["objects_only_in_" + b]))
