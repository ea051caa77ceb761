#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds of the kernel library, symbol by symbol (no GPU).

    python scripts/kernel_diff.py OLD/_llmc_hip*.so NEW/_llmc_hip*.so

For every kernel in both: the instruction bytes of its function, and the registers, LDS and scratch its
descriptor's metadata records. Prints the counts, the kernels only one side has (grouped by template) and
every kernel that differs; exit status 1 if a shared kernel differs or NEW has a kernel OLD lacks. A refactor
of host code must leave every kernel as it was (profiles/r15_gemv_geometry.md).
"""

import collections
import hashlib
import os
import re
import subprocess
import sys
import tempfile

TOOLS = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
META = (".sgpr_count", ".vgpr_count", ".agpr_count", ".sgpr_spill_count", ".vgpr_spill_count",
        ".group_segment_fixed_size", ".private_segment_fixed_size", ".kernarg_segment_size", ".max_flat_workgroup_size")


def code_objects(lib: str, d: str):
    fb = os.path.join(d, "fatbin")
    subprocess.run([f"{TOOLS}/llvm-objcopy", f"--dump-section=.hip_fatbin={fb}", lib], check=True)
    data = open(fb, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    offs, i = [], data.find(magic)
    while i >= 0:
        offs.append(i)
        i = data.find(magic, i + 1)
    for k, o in enumerate(offs):
        bundle, co = os.path.join(d, f"b{k}"), os.path.join(d, f"c{k}.elf")
        with open(bundle, "wb") as f:
            f.write(data[o:offs[k + 1] if k + 1 < len(offs) else len(data)])
        r = subprocess.run([f"{TOOLS}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={bundle}",
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], capture_output=True)
        if r.returncode == 0 and os.path.getsize(co) > 0:
            yield co


def kernels(lib: str) -> dict:
    """{kernel name: (sha1 of its code bytes, metadata tuple)}"""
    res = {}
    with tempfile.TemporaryDirectory() as d:
        for co in code_objects(lib, d):
            notes = subprocess.run([f"{TOOLS}/llvm-readelf", "--notes", co], capture_output=True, text=True).stdout
            meta, cur = {}, {}

            def flush():
                if ".symbol" in cur:
                    meta[cur[".symbol"][:-3]] = tuple(cur.get(k) for k in META)

            for ln in notes.splitlines():  # a kernel's keys are sorted: .agpr_count opens its entry
                ln = ln.strip()
                if ln.startswith("- .agpr_count"):
                    flush()
                    cur = {}
                ln = ln.lstrip("- ")
                key, _, val = ln.partition(":")
                if key in META:
                    cur[key] = int(val)
                elif key == ".symbol":
                    cur[key] = val.strip()
            flush()
            syms = subprocess.run([f"{TOOLS}/llvm-readelf", "-sW", "-S", co], capture_output=True, text=True).stdout
            text_addr = text_off = None
            for ln in syms.splitlines():
                m = re.match(r"\s*\[\s*\d+\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)", ln)
                if m:
                    text_addr, text_off = int(m.group(1), 16), int(m.group(2), 16)
            blob = open(co, "rb").read()
            for ln in syms.splitlines():
                f = ln.split()
                if len(f) == 8 and f[3] == "FUNC" and f[7] in meta:
                    a, n = int(f[1], 16), int(f[2])
                    code = blob[text_off + a - text_addr:text_off + a - text_addr + n]
                    res[f[7]] = (hashlib.sha1(code).hexdigest(), meta[f[7]])
    return res


def main() -> int:
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    both = sorted(set(old) & set(new))
    differ = [k for k in both if old[k] != new[k]]
    print(f"kernels: old {len(old)}, new {len(new)}, in both {len(both)}; {len(both) - len(differ)} of {len(both)} identical")
    demangle = lambda names: subprocess.run(["c++filt"], input="\n".join(names), capture_output=True,
                                            text=True).stdout.splitlines()
    for title, names in (("only in old", sorted(set(old) - set(new))), ("only in new", sorted(set(new) - set(old)))):
        groups = collections.Counter(re.sub(r"<.*", "", n) for n in demangle(names))
        print(f"{title}: {len(names)}", dict(groups))
        if "-v" in sys.argv:
            print("\n".join("  " + n for n in demangle(names)))
    for k in differ:
        print("DIFFERS:", demangle([k])[0], old[k], new[k])
    assert all(None not in v[1] for v in list(old.values()) + list(new.values())), "metadata not parsed"
    return 1 if differ or set(new) - set(old) else 0


if __name__ == "__main__":
    sys.exit(main())
