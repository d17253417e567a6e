"""Is the gfx950 device code of every csrc/*.hip the same as in another tree?  No GPU needed.

    git worktree add ../parent HEAD~1
    python tools/device_asm_identity.py ../parent [FILE.hip ...]

Compiles each source of both trees to device assembly with build.py's FLAGS (plus
-S --cuda-device-only), drops the lines that carry the per-compilation random __hip_cuid_ symbol,
and compares what is left as whole texts, by SHA-256.  Prints same / differs per file and, for a
full run, writes profiles/mlp_frag_asm_identity.json.  Exit status 1 when any file differs.
"""
import hashlib
import importlib.util
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "3dioumatch_amd"
spec = importlib.util.spec_from_file_location("pn2_build", os.path.join(ROOT, PKG, "build.py"))
pn2_build = importlib.util.module_from_spec(spec)
spec.loader.exec_module(pn2_build)


def digest(tree, name):
    # relative source path, run from the tree's root: nothing of the tree's location reaches the text
    asm = subprocess.check_output(
        [pn2_build.HIPCC, *pn2_build.FLAGS, "-S", "--cuda-device-only",
         os.path.join(PKG, "csrc", name), "-o", "-"], cwd=tree, stderr=subprocess.DEVNULL)
    kept = [line for line in asm.split(b"\n") if b"__hip_cuid_" not in line]
    return hashlib.sha256(b"\n".join(kept)).hexdigest()


def hip_sources(tree):
    return {f for f in os.listdir(os.path.join(tree, PKG, "csrc")) if f.endswith(".hip")}


def main(argv):
    if len(argv) < 2:
        sys.exit(__doc__)
    parent = os.path.abspath(argv[1])
    both = hip_sources(ROOT) & hip_sources(parent)
    only = sorted(hip_sources(ROOT) ^ hip_sources(parent))
    names = sorted(argv[2:] or both)
    with ThreadPoolExecutor(max_workers=8) as ex:
        new = ex.map(lambda n: digest(ROOT, n), names)
        old = ex.map(lambda n: digest(parent, n), names)
        rows = [{"file": n, "parent_sha256": o, "sha256": d, "verdict": "same" if o == d else "differs"}
                for n, o, d in zip(names, old, new)]
    for r in rows:
        print("%-8s %s" % (r["verdict"], r["file"]))
    for n in only:
        print("%-8s %s" % ("one-tree", n))
    bad = [r["file"] for r in rows if r["verdict"] != "same"] + only
    if not argv[2:]:
        out = os.path.join(ROOT, "profiles", "mlp_frag_asm_identity.json")
        with open(out, "w") as f:
            json.dump({"flags": pn2_build.FLAGS + ["-S", "--cuda-device-only"], "dropped_lines": "__hip_cuid_",
                       "files_in_one_tree_only": only, "files": rows}, f, indent=1)
            f.write("\n")
    print("%d of %d files differ" % (len(bad), len(rows) + len(only)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
