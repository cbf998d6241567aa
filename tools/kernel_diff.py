#!/usr/bin/env python3
"""Compare the gfx950 device code of two csrc trees kernel by kernel (CPU only).

usage: tools/kernel_diff.py OLD_CSRC NEW_CSRC [--map OLD_MANGLED=NEW_MANGLED ...]

Every .hip of each tree is compiled with the Makefile's flags, device side only.  Kernels are matched by mangled name, whichever
file they live in (--map pairs a kernel whose template signature changed); rocPRIM's are ignored.  Prints one line per kernel --
identical or different, with its resource metadata and instruction count -- and the kernels present on one side only (the first differing lines of a
kernel go to stderr); exits 1 on any difference."""
import difflib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
FLAGS = "-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -I/opt/rocm/include -x hip".split()
META = [".vgpr_count", ".sgpr_count", ".agpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
        ".kernarg_segment_size", ".max_flat_workgroup_size"]


def kernels_of(src, tmp):
    """{mangled name: (instruction lines, {metadata})} of one .hip file"""
    obj = os.path.join(tmp, re.sub(r"\W", "_", src) + ".o")
    subprocess.check_call([HIPCC] + FLAGS + ["--cuda-device-only", "--no-gpu-bundle-output", "-I", os.path.dirname(src), "-c", src, "-o", obj])
    notes = subprocess.check_output([LLVM + "/llvm-readelf", "--notes", obj], text=True)
    meta = {}
    for entry in re.split(r"\n\s+- \.agpr_count:", "\n" + notes)[1:]:
        entry = "  - .agpr_count:" + entry
        name = re.search(r"^\s+\.name:\s+(\S+)", entry, re.M).group(1)
        meta[name] = {k: int(re.search(r"\s" + re.escape(k) + r":\s+(\d+)", entry).group(1)) for k in META}
    text, cur, pcrel = {}, None, 0
    for line in subprocess.check_output([LLVM + "/llvm-objdump", "-d", "--no-show-raw-insn", obj], text=True).splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
        if m:
            cur = text.setdefault(m.group(1), []) if m.group(1) in meta else None
        elif cur is not None and line.strip():
            ins = re.sub(r"\s*//.*$", "", line).strip()                  # "// addr: <sym+off>" trailers off: addresses are in them ...
            # ... and in the distance from the kernel to a global (__constant__ table) that the two adds behind s_getpc_b64 carry:
            # it changes with the other code of the file, not with the kernel
            if pcrel and re.match(r"s_addc?_u32 ", ins):
                ins, pcrel = re.sub(r",\s*\S+$", ", <pc-relative>", ins), pcrel - 1
            else:
                pcrel = 2 if ins.startswith("s_getpc_b64") else 0
            cur.append(ins)
    for lines in text.values():                                          # the padding behind a file's last kernel is not its code
        while lines and lines[-1] in ("s_nop 0", "s_code_end", "..."):
            lines.pop()
    return {k: (text.get(k, []), meta[k]) for k in meta if "rocprim" not in k}


def tree(csrc, tmp):
    srcs = sorted(os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".hip"))
    out = {}
    with ThreadPoolExecutor(8) as ex:
        for src, ks in zip(srcs, ex.map(lambda s: kernels_of(s, tmp), srcs)):
            for k, v in ks.items():
                out[k] = v + (os.path.basename(src),)
    return out


def main():
    args = [a for a in sys.argv[1:] if a != "--map" and "=" not in a]
    if len(args) != 2:
        sys.exit(__doc__)
    renamed = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
    with tempfile.TemporaryDirectory() as t_old, tempfile.TemporaryDirectory() as t_new:
        old, new = tree(args[0], t_old), tree(args[1], t_new)
    old = {renamed.get(k, k): v for k, v in old.items()}
    demangle = lambda ks: dict(zip(ks, subprocess.check_output(["c++filt"] + list(ks), text=True).splitlines())) if ks else {}
    names = demangle(sorted(set(old) | set(new)))
    short = lambda k: re.sub(r"\(.*", "", names[k]).replace("void ", "")
    differ = 0
    for k in sorted(set(old) & set(new), key=lambda k: (new[k][2], short(k))):
        (ta, ma, fa), (tb, mb, fb) = old[k], new[k]
        same = ta == tb and ma == mb
        differ += not same
        fmt = lambda m: " ".join("%s=%d" % (q.strip(".").replace("_count", "").replace("_segment_fixed_size", "").replace("_segment_size", "").replace("_flat_workgroup_size", "_wg"), m[q]) for q in META)
        insts = "insts=%d" % len(tb) if len(ta) == len(tb) else "insts=%d -> %d" % (len(ta), len(tb))
        print("%-9s %-34s %s -> %s  %s %s" % ("identical" if same else "DIFFERENT", short(k), fa, fb, fmt(mb) if ma == mb else fmt(ma) + "  ->  " + fmt(mb), insts))
        if ta != tb:
            for d in list(difflib.unified_diff(ta, tb, "old", "new", n=0, lineterm=""))[2:42]:
                print("          " + d, file=sys.stderr)
    for side, only in (("old", set(old) - set(new)), ("new", set(new) - set(old))):
        for k in sorted(only, key=short):
            print("%s only  %s (%s)" % (side, names[k], (old if side == "old" else new)[k][2]))
    differ += len(set(old) ^ set(new))
    print("%d kernels compared, %d differences" % (len(set(old) & set(new)), differ))
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
