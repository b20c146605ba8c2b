"""Compare the device code of two builds of one HIP source, kernel by kernel.

    hipcc <the library's flags> -save-temps=obj -Rpass-analysis=kernel-resource-usage -c FILE.hip -o DIR/FILE.o 2> DIR/build.log
    python tools/isa_diff.py PARENT_DIR BRANCH_DIR FILE

reads DIR/FILE-hip-amdgcn-amd-amdhsa-gfx950.s of both sides, splits it into the symbols with a body
(`.type NAME,@function` .. `.Lfunc_end`), drops comments, directives and blank lines, renumbers the
local labels (.LBB<function>_<block> -> .LBB_<block>: a function's number is its position in the file)
and compares the instruction streams of every symbol the parent has.  The resource rows (every
kernel-resource-usage remark of a kernel, from build.log) are compared the same way.  Prints a summary;
exit status 1 if a parent symbol is missing from the branch or differs.
"""
import re
import sys


def functions(path):
    out, name, body = {}, None, []
    for line in open(path, errors="replace"):
        m = re.match(r"\s*\.type\s+([^,\s]+),@function", line)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if re.match(r"\s*\.Lfunc_end\d+:", line):
            out[name] = body
            name = None
            continue
        s = line.split(";")[0].strip()
        if not s or s.startswith(".") and not s.startswith(".LBB") or s == name + ":":
            continue
        body.append(re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", s))
    return out


def resources(path):
    out, name = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: [^ ]+ +(.*?) \[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m:
            continue
        row = m.group(1).strip()
        if row.startswith("Function Name:"):
            name = row.split(":", 1)[1].strip()
            out[name] = []
        elif name:
            out[name].append(row)
    return out


def main():
    parent, branch, src = sys.argv[1:4]
    stem = src.rsplit(".", 1)[0] + "-hip-amdgcn-amd-amdhsa-gfx950.s"
    a, b = functions(f"{parent}/{stem}"), functions(f"{branch}/{stem}")
    common = [n for n in a if n in b]
    missing = [n for n in a if n not in b and not n.startswith("__hip_cuid")]
    differ = [n for n in common if a[n] != b[n]]
    new = [n for n in b if n not in a and not n.startswith("__hip_cuid")]
    print(f"{src}: functions parent {len(a)} branch {len(b)} common {len(common)}, parent functions missing from the branch "
          f"{len(missing)}, with a different instruction stream {len(differ)}, new in the branch {len(new)}; instructions "
          f"parent {sum(map(len, a.values()))} branch {sum(map(len, b.values()))} (new functions {sum(len(b[n]) for n in new)})")
    ra, rb = resources(f"{parent}/build.log"), resources(f"{branch}/build.log")
    rdiff = [n for n in ra if rb.get(n) != ra[n]]
    print(f"{src}: kernel-resource-usage rows parent {sum(map(len, ra.values()))} of {len(ra)} kernels, branch "
          f"{sum(map(len, rb.values()))} of {len(rb)} kernels; parent kernels with a different row {len(rdiff)}")
    for n in (missing + differ + rdiff)[:20]:
        print("  DIFFERS", n)
    if "--new" in sys.argv:
        for n in new:
            print("  new", n, len(b[n]), "instructions;", "; ".join(rb.get(n, [])))
    return 1 if missing or differ or rdiff else 0


if __name__ == "__main__":
    sys.exit(main())
