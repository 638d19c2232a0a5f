"""Compare the device code of two builds of one kernel file, kernel by kernel (no GPU needed).
usage: python tools/device_code_diff.py A.s B.s, with A.s and B.s from
  hipcc <the flags of tools/resource_usage.sh, without the remark option> --cuda-device-only -S -o A.s abc_amd/csrc/abc_kernels_X.hip
Prints the kernels only one file has and the kernels whose text differs; exit status 1 if there are any.  A kernel is everything
from its "Begin function" marker to the next one (code, resource comments aside, kernel descriptor).  Comments, the numbers of
compiler-local labels (.LBB12_3: they count functions in emission order) and the per-build __hip_cuid_ symbol are set aside, so a
change in emission order alone compares equal.  A plain text comparison: the resource table of tools/resource_usage.sh cannot
see a change at equal register count, this can."""
import re
import sys


def kernels(path):
    out, name = {}, None
    for line in open(path):
        m = re.search(r"; -- Begin function (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = []
        elif line.startswith("\t.amdgpu_metadata") or line.startswith("\t.ident"):  # behind the last kernel: the file's own tail
            name = None
        elif name and line.startswith("\t.p2alignl"):  # the padding behind the file's last kernel opens that tail (".text" before it)
            if out[name] and out[name][-1] == ".text":
                out[name].pop()
            name = None
        text = re.sub(r"(\.L[A-Za-z_]+?)\d+", r"\1", line.split(";")[0]).strip()
        # a ".section .text.<kernel>" line opens the NEXT kernel's section, ahead of its marker: emission order again
        if name and text and "__hip_cuid_" not in text and not text.startswith(".section\t.text"):
            out[name].append(text)
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    only = [(sys.argv[1 + (k in b)], k) for k in sorted(a.keys() ^ b.keys())]
    differ = [k for k in sorted(a.keys() & b.keys()) if a[k] != b[k]]
    for path, k in only:
        print("only in %s: %s" % (path, k))
    for k in differ:
        print("differs: %s" % k)
    print("%d kernels in %s, %d in %s: %d on one side only, %d differ" % (len(a), sys.argv[1], len(b), sys.argv[2], len(only), len(differ)))
    sys.exit(1 if only or differ else 0)


if __name__ == "__main__":
    main()
