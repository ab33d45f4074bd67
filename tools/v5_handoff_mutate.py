#!/usr/bin/env python3
"""Evidence that tools/v5_handoff_check.py bites (dev tool, CPU only): six one-line mutations of the comb walker's hand-off,
each in a scratch copy of the tree that is compiled to assembly and linted there -- never loaded, never run.  Every mutation has
to fail with the rule that belongs to it, the unmutated copy has to pass.

  python tools/v5_handoff_mutate.py [out.txt]       the table of profiles/v5_handoff_lint.txt; exit status 1 if a row is wrong
"""
import concurrent.futures, os, re, shutil, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V5, DEV = "stereo_matching_cuda_amd/csrc/smx_agg_v5.hip", "stereo_matching_cuda_amd/csrc/smx_agg_dev.h"
WAIT = re.compile(r'( *asm volatile\("s_waitcnt lgkmcnt\(0\)" : "\+v"\(r2\[0\]\)[^;]*;\n)( *if \(lane == 0\) __hip_atomic_fetch_add\(&s_x1,[^\n]*\n)')

# (name, file, what to replace: text or pattern, by what, the rule that has to fire)
MUTATIONS = [
    ("none", None, None, None, None),
    ("S2_KEEP 12 -> 13", V5, "constexpr int S2_KEEP = 12;", "constexpr int S2_KEEP = 13;", "R1"),
    ("KEEP without - BH / 2", V5, "QPERM ? S2_KEEP - BH / 2 : S2_KEEP;", "QPERM ? S2_KEEP : S2_KEEP;", "R1"),
    ("lgkmcnt(0) behind the s_x1 add", V5, WAIT, r"\2\1", "R4"),
    ("st16_sc1 without AUX_SC1", DEV, "r, (int)byteoff, 0, AUX_SC1);", "r, (int)byteoff, 0, 0);", "R5"),
    ("ld16_sc1 without AUX_SC1", DEV, "(r, (int)byteoff, 0, AUX_SC1));", "(r, (int)byteoff, 0, 0));", "R5"),
    ("one interior q store (T0 = 8) removed", V5, "const bool va = !BORDER ||", "const bool va = (!BORDER && T0 != 8) || BORDER &&", "R1"),
]


def run(m):
    name, path, old, new, rule = m
    with tempfile.TemporaryDirectory() as td:
        tree = os.path.join(td, "tree")
        for d in ("tools", "include", "stereo_matching_cuda_amd/csrc"):            # all that the lint and its compile read
            shutil.copytree(os.path.join(ROOT, d), os.path.join(tree, d), ignore=shutil.ignore_patterns("__pycache__", "ubench"))
        if path:
            text = open(os.path.join(tree, path)).read()
            mutated, n = old.subn(new, text) if hasattr(old, "subn") else (text.replace(old, new), text.count(old))
            assert n == 1, f"{name}: the text to mutate occurs {n} times in {path}"
            open(os.path.join(tree, path), "w").write(mutated)
        p = subprocess.run([sys.executable, os.path.join(tree, "tools", "v5_handoff_check.py")], capture_output=True, text=True)
    found = [l for l in p.stdout.split("\n") if l.startswith("FINDING")]
    rules = sorted({l.split()[1] for l in found})
    first = next((l for l in found if l.split()[1] == rule), found[0] if found else "")
    ok = p.returncode == (1 if rule else 0) and (rule in rules if rule else not found)
    return name, rule or "-", p.returncode, rules, len(found), re.sub(r"_ZN3smx2v59k_v5_walkILi(\d)ELi(\d)EEEvNS0_4ArgsE", r"k_v5_walk<\1,\2>", first), ok


def main(argv):
    with concurrent.futures.ThreadPoolExecutor(max_workers=4) as ex:
        rows = list(ex.map(run, MUTATIONS))
    out = ["v5_handoff_check.py on scratch copies of the tree, one mutation each (compiled to assembly only; tools/v5_handoff_mutate.py)", "",
           "mutation | rule expected | exit status | rules that fired (findings) | first finding of the expected rule", "---|---|---|---|---"]
    for name, rule, rc, rules, n, first, ok in rows:
        out.append(f"{name} | {rule} | {rc} | {', '.join(rules) or '-'} ({n}) | {first or '-'}" + ("" if ok else "   <-- WRONG"))
    text = "\n".join(out) + "\n"
    print(text, end="")
    if argv:
        open(argv[0], "w").write(text)
    return 0 if all(r[-1] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
