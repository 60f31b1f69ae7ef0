"""Two builds of nbk.hip compared kernel by kernel in their gfx950 assembly: for a refactor that must not move generated code.

    python tools/kernel_diff.py OLD.s NEW.s [--mark substring] [--old-digest D] [--new-digest D] > profiles/NAME.txt

OLD.s / NEW.s: `hipcc -S --cuda-device-only` of the two trees with build.py's flags (what tools/kernel_resources.py compiles).  Per
kernel: "identical" when the instruction text of its body is the same (block labels renumbered, comments dropped), else the
register / scratch / occupancy rows of both from the compiler's summary.  Kernels whose name holds --mark are listed one by one, the
rest are counted.  Exit status 1 when a kernel outside --mark differs or a kernel exists on one side only."""
import argparse
import re
import subprocess
import sys

SUMMARY = re.compile(r"^\s*\.amdhsa_kernel (\S+)$(.*?)^; Occupancy: (\d+)", re.M | re.S)


def kernels(path):
    """{demangled name: (body text, (vgpr, agpr, total, scratch, occupancy))} of one assembly file."""
    txt = open(path).read()
    out = {}
    for m in SUMMARY.finditer(txt):
        sym, info = m.group(1), m.group(2)
        g = lambda k: int(re.search(rf"; {k}: (\d+)", info).group(1))          # noqa: E731
        a = txt.index(f"\n{sym}:")
        body = txt[a:txt.index(".Lfunc_end", a)]
        body = re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\s*;.*", "", body))
        name = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip().split("(")[0]
        out[name] = (body, (g("NumVgprs"), g("NumAgprs"), g("TotalNumVgprs"), g("ScratchSize"), int(m.group(3))))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--mark", default="k_cloud")
    ap.add_argument("--old-digest", default="?")
    ap.add_argument("--new-digest", default="?")
    a = ap.parse_args()
    old, new = kernels(a.old), kernels(a.new)
    print(f"# kernel_diff.py  old: kernels {a.old_digest}  new: kernels {a.new_digest}  ({len(old)} / {len(new)} kernels)")
    bad = sorted(set(old) ^ set(new))
    for name in bad:
        print(f"{name}: only in the {'old' if name in old else 'new'} build")
    row = lambda r: "vgpr %3d  agpr %3d  total %3d  scratch %5d B  occupancy %d" % r          # noqa: E731
    same_rest = 0
    for name in sorted(set(old) & set(new)):
        same = old[name][0] == new[name][0]
        if a.mark not in name:
            same_rest += same
            if same:
                continue
            bad.append(name)
        if same:
            print(f"{name}: identical   ({row(new[name][1])})")
        else:
            print(f"{name}: instruction text differs\n    old  {row(old[name][1])}\n    new  {row(new[name][1])}")
    print(f"kernels without '{a.mark}' in their name: {same_rest} identical, {len([n for n in bad if n in old and n in new])} different")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
