"""Compare two device assembly listings (hipcc --cuda-device-only -S) kernel by kernel: for every kernel symbol both listings
define, are the instruction streams identical?  Kernels only one of them defines are listed with their register counts.

    python tools/isa_kernel_diff.py before.s after.s [substring the kernel names must contain] [--rename REGEX REPL]...

--rename: applied to the kernel names of `after` before they are matched (a kernel that gained a defaulted template parameter has a
new mangled name for the same instantiation).

Labels and comments are dropped and local label numbers are renamed in order of appearance, so a listing that only gained
other kernels compares equal.  Used for DESIGN.md section 6s: the smooth-Q template parameter leaves the existing
instantiations of the fp8 attention kernels as they were."""
import re
import sys


def kernels(path):
    out, name, body, meta = {}, None, [], {}
    for line in open(path):
        m = re.match(r"^(_Z\w+):\s*(;.*)?$", line)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = (body, meta.setdefault(name, {}))
            name = None
            continue
        text = line.split(";")[0].strip()
        if text and not text.startswith("."):
            body.append(text)
        elif text.startswith(".L") and text.endswith(":"):
            body.append(text)
    # register counts from the .amdhsa directives
    cur = None
    for line in open(path):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\w+)", line)
        if m:
            cur = m.group(1)
        m = re.match(r"\s*\.amdhsa_next_free_(vgpr|sgpr)\s+(\d+)", line)
        if m and cur in out:
            out[cur][1][m.group(1)] = int(m.group(2))
        m = re.match(r"\s*\.amdhsa_private_segment_fixed_size\s+(\d+)", line)
        if m and cur in out:
            out[cur][1]["scratch"] = int(m.group(1))
    return out


def canon(body):
    names = {}
    res = []
    for text in body:
        def sub(m):
            return names.setdefault(m.group(0), f".L{len(names)}")
        res.append(re.sub(r"\.L[\w$]+", sub, text))
    return res


def main():
    argv = sys.argv[1:]
    renames = []
    while "--rename" in argv:
        i = argv.index("--rename")
        renames.append((argv[i + 1], argv[i + 2]))
        del argv[i:i + 3]
    a, b = kernels(argv[0]), kernels(argv[1])
    want = argv[2] if len(argv) > 2 else ""
    for pat, repl in renames:
        b = {re.sub(pat, repl, name): v for name, v in b.items()}
    same = diff = 0
    for name in sorted(a):
        if want not in name or name not in b:
            continue
        if canon(a[name][0]) == canon(b[name][0]):
            same += 1
        else:
            diff += 1
            print(f"DIFFERENT  {name}  {len(a[name][0])} -> {len(b[name][0])} lines")
    print(f"{same} kernels identical, {diff} different")
    for name in sorted(b):
        if want in name and name not in a:
            print(f"new  {name}  {b[name][1]}  {len(b[name][0])} lines")
    for name in sorted(a):
        if want in name and name not in b:
            print(f"gone {name}")
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
