"""Are the kernels of one .hip file the same instruction streams in two builds?  Takes two device assembly files of the same source
at two commits (hipcc <build.py's FLAGS> --cuda-device-only -S file.hip -o x.s), demangles the kernel names, drops labels, directives
and comments, and compares kernel by kernel.  A template that gained trailing defaulted parameters is matched by --strip-args N:
that many trailing template arguments equal to `false` are dropped from the names of the second file; a function that became a
template is matched by --map 'NAME IN THE SECOND FILE=NAME IN THE FIRST' (demangled, as this tool prints them).  Needs no GPU.
    python tools/isa_compare.py before.s after.s [--strip-args 1] [--map 'void vj::atlas_pack<false>(vj::AtlasPackArgs)=vj::atlas_pack(vj::AtlasPackArgs)']"""
import argparse
import re
import subprocess


def kernels(path):
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
            cur = out.setdefault(name, [])
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        if cur is not None:
            code = line.split(";")[0].strip()
            if code and not code.startswith("."):
                cur.append(re.sub(r"\.LBB\d+_", ".LBB_", code))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--strip-args", type=int, default=0)
    ap.add_argument("--map", action="append", default=[], metavar="AFTER=BEFORE")
    args = ap.parse_args()
    b, a = kernels(args.before), kernels(args.after)
    for _ in range(args.strip_args):
        a = {re.sub(r", false>\(", ">(", k): v for k, v in a.items()}
    for m in args.map:
        after, before = m.split("=", 1)
        a[before] = a.pop(after)
    same = [k for k in b if a.get(k) == b[k]]
    for k in b:
        if k not in a:
            print("missing in the second file:", k)
        elif a[k] != b[k]:
            print(f"DIFFERENT ({len(b[k])} / {len(a[k])} instructions):", k)
    print(f"{len(same)} of {len(b)} kernels identical, {len(a) - len(set(a) & set(b))} only in the second file")


if __name__ == "__main__":
    main()
