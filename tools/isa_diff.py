#!/usr/bin/env python3
"""Per-kernel comparison of the gfx950 ISA that `make` leaves beside the objects, for the DP launcher files:
    python3 tools/isa_diff.py <build directory of the parent> <build directory of this tree>
Kernels are matched by name (instantiation order may move them within a file); labels are compared without the
function's ordinal.  Prints per file the kernels that are missing, new or different and a digest of each; exit 1 on any."""
import re, sys, hashlib
FILES = ["is_k_unary", "is_k_unary_fast", "is_k_unary_path", "is_k_pairwise", "is_k_prepare", "is_k_backtrace",
         "is_k_head", "is_k_head_backward", "is_k_road", "is_k_frontend"]
SUF = "-hip-amdgcn-amd-amdhsa-gfx950.s"

def kernels(path):
    lines = open(path).read().split("\n")
    names = [l.split()[1] for l in lines if l.startswith("\t.amdhsa_kernel ") or l.strip().startswith(".amdhsa_kernel ")]
    out = {}
    cur = None
    for l in lines:
        if cur is None:
            head = l.split(":")[0]
            if l.startswith("_Z") and ":" in l and head in names and head not in out:
                cur = head
                out[cur] = []
        else:
            # function-order dependent local label numbers
            out[cur].append(re.sub(r"[ \t]+", " ", re.sub(r"\bBB\d+_", "BBN_", re.sub(r"\.L(BB|func_end|func_begin|tmp)\d+", r".L\1N", l))))
            if l.strip() == ".end_amdhsa_kernel":
                cur = None
    return {k: "\n".join(v) for k, v in out.items()}

def main(parent, branch):
    bad = 0
    for f in FILES:
        a, b = kernels(f"{parent}/{f}{SUF}"), kernels(f"{branch}/{f}{SUF}")
        gone, new = sorted(set(a) - set(b)), sorted(set(b) - set(a))
        diff = [k for k in a if k in b and a[k] != b[k]]
        bad += len(gone) + len(new) + len(diff)
        print(f"{f}: kernels parent {len(a)} branch {len(b)}; missing {len(gone)}, new {len(new)}, ISA differs {len(diff)}")
        for k in gone: print("  MISSING", k)
        for k in new: print("  NEW", k)
        for k in diff: print("  DIFFERS", k)
        for k in sorted(a):
            if k in b:
                print(f"  {hashlib.sha256(a[k].encode()).hexdigest()[:16]} {hashlib.sha256(b[k].encode()).hexdigest()[:16]} "
                      f"{len(a[k].splitlines()):6d} lines  {k}")
    print("RESULT:", "identical" if bad == 0 else f"{bad} defects")
    return bad

if __name__ == "__main__":
    sys.exit(1 if main(sys.argv[1], sys.argv[2]) else 0)
