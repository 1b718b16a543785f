"""No GPU needed: one line per kernel of every translation unit of the library (rpsmf_amd/build.py: _units()) with the numbers the
code object carries and a digest of the kernel's instructions -- the recipe of profiles/README.md for the *_kernel_metadata_*.txt files:

    python tools/kernel_metadata.py > profiles/capi_kernel_metadata_NAME.txt

Compiles the device side of each unit with the flags of rpsmf_amd/build.py plus --cuda-device-only, unbundles it if the compiler bundled
it, and reads `llvm-readelf --notes` (the AMDGPU metadata), `llvm-readelf -sW` (the size of each kernel's code) and
`llvm-objdump -d --no-show-raw-insn --no-leading-addr --disassemble-symbols=NAME` (the instructions, trailing `// ADDR:` comments
and the alignment padding behind the last instruction stripped; the column is the first 16 hex digits of their SHA-256).  Two builds whose digests agree for a kernel run the same
instructions there.  Sorted by mangled name; a kernel that more than one unit instantiates has a line per unit."""

import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LLVM = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/llvm/bin")

FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size", ".kernarg_segment_size",
          ".max_flat_workgroup_size")


def unit_kernels(obj, tmp):
    """{kernel: metadata fields + [code bytes, digest]} of one device object"""
    with open(obj, "rb") as f:
        bundled = f.read(24).startswith(b"__CLANG_OFFLOAD_BUNDLE__")
    if bundled:
        elf = os.path.join(tmp, os.path.basename(obj) + ".elf")
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o",
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={obj}", f"--output={elf}"])
        obj = elf
    notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", obj], text=True)
    syms = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "-sW", obj], text=True)
    size = {}
    for line in syms.splitlines():
        p = line.split()
        if len(p) >= 8 and p[3] == "FUNC":
            size[p[7]] = int(p[2], 0)
    kernels = {}
    for block in re.split(r"\n\s*- \.agpr_count:", "\n" + notes)[1:]:
        block = "  - .agpr_count:" + block
        name = re.search(r"^\s*\.name:\s*(\S+)\s*$", block, flags=re.M).group(1)
        vals = [int(re.search(r"^\s*(?:- )?" + re.escape(f) + r":\s*(\d+)", block, flags=re.M).group(1)) for f in FIELDS]
        kernels[name] = vals + [size.get(name, -1)]
    if kernels:
        dis = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr",
                                       "--disassemble-symbols=" + ",".join(sorted(kernels)), obj], text=True)
        body = {}
        cur = None
        for line in dis.splitlines():
            m = re.match(r"^<(\S+)>:$", line)
            if m:
                cur = m.group(1)
                body[cur] = []
            elif cur is not None and line.strip():
                body[cur].append(re.sub(r"\s*//\s*[0-9A-Fa-f]+:.*$", "", line).strip())
        for name in kernels:
            while body[name] and body[name][-1] in ("s_nop 0", "s_code_end", "..."):      # padding up to the next symbol's alignment
                body[name].pop()
            kernels[name].append(hashlib.sha256("\n".join(body[name]).encode()).hexdigest()[:16])
    return kernels


def main():
    from rpsmf_amd import build

    objs = sys.argv[1:]          # already compiled device objects (default: compile every unit)
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        if not objs:
            for obj_name, src, _deps, extra in build._units():
                obj = os.path.join(tmp, obj_name.replace(".o", "_dev.o"))
                subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + build.FLAGS + extra + ["-I", os.path.join(ROOT, "include"),
                                       "--cuda-device-only", "-c", src, "-o", obj])
                objs.append(obj)
        for obj in objs:
            rows += sorted(unit_kernels(obj, tmp).items())
    rows.sort(key=lambda kv: kv[0])
    print("# kernel  vgpr agpr sgpr private_segment group_segment kernarg max_flat_workgroup code_bytes instructions_sha256")
    for name, vals in rows:
        print(name, *vals)
    print(f"# {len(rows)} kernels, {sum(v[3] > 0 for _, v in rows)} with private segment > 0, "
          f"{sum(v[0] == 512 for _, v in rows)} at 512 VGPRs")


if __name__ == "__main__":
    main()
