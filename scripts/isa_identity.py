"""Per-kernel comparison of two device assembly files of one source (hipcc -S --cuda-device-only, gfx950).

    python scripts/isa_identity.py PARENT.s NEW.s [LABEL]

Instruction text per kernel with comments dropped and basic-block / jump-table label numbers normalised (they are numbered per
file).  Prints the summary kept under profiles/*/isa_identity.txt: counts, then the kernels that differ, were added or removed.
"""
import re
import shutil
import subprocess
import sys


def kernels(path):
    text = open(path).read()
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M))
    out = {}
    for name in names:
        m = re.search(r"^%s:.*?\n(.*?)^\.Lfunc_end\d+:" % re.escape(name), text, flags=re.M | re.S)
        if not m:
            continue
        body = m.group(1)
        lines, labels = [], {}

        def norm(mm):
            return labels.setdefault(mm.group(0), "L%d" % len(labels))
        for line in body.split("\n"):
            line = line.split(";")[0].strip()
            if not line or line.startswith(".p2align") or line.startswith(".loc") or line.startswith(".cfi"):
                continue
            lines.append(re.sub(r"\.L(?:BB|JTI)\d+_\d+", norm, line))
        out[name] = "\n".join(lines)
    return out


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    try:
        res = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, res))
    except Exception:
        return {n: n for n in names}


if __name__ == "__main__":
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    label = sys.argv[3] if len(sys.argv) > 3 else ""
    same = [k for k in a if k in b and a[k] == b[k]]
    diff = [k for k in a if k in b and a[k] != b[k]]
    added = [k for k in b if k not in a]
    removed = [k for k in a if k not in b]
    dm = demangle(diff + added + removed)
    print("%sparent kernels %d new kernels %d identical %d different %d" % (label + ": " if label else "", len(a), len(b), len(same), len(diff)))
    for title, ks in (("different", diff), ("added", added), ("removed", removed)):
        if ks:
            print(title + ":")
            for line in sorted(dm[k] for k in ks):
                print("  " + line)
