"""No GPU needed: one line per kernel of the C-ABI translation unit (psmf_capi.hip and what it includes) with the numbers the code
object carries -- the recipe of profiles/README.md for the capi_kernel_metadata_*.txt files:

    python tools/kernel_metadata.py > profiles/capi_kernel_metadata_NAME.txt

Compiles the device side with the flags of rpsmf_amd/build.py plus --cuda-device-only, unbundles it if the compiler bundled it, and
reads `llvm-readelf --notes` (the AMDGPU metadata) and `llvm-readelf -sW` (the size of each kernel's code).  Sorted by mangled name."""

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


def main():
    from rpsmf_amd import build

    obj_in = sys.argv[1] if len(sys.argv) > 1 else None          # an already compiled device object
    with tempfile.TemporaryDirectory() as tmp:
        obj = obj_in or os.path.join(tmp, "capi_dev.o")
        if not obj_in:
            subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + build.FLAGS + ["-I", os.path.join(ROOT, "include"),
                                   "--cuda-device-only", "-c", os.path.join(build.CSRC, "psmf_capi.hip"), "-o", obj])
        with open(obj, "rb") as f:
            bundled = f.read(24).startswith(b"__CLANG_OFFLOAD_BUNDLE__")
        if bundled:
            elf = os.path.join(tmp, "capi_dev.elf")
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
        kernels[name] = vals
    print("# kernel  vgpr agpr sgpr private_segment group_segment kernarg max_flat_workgroup code_bytes")
    for name in sorted(kernels):
        print(name, *kernels[name], size.get(name, -1))
    print(f"# {len(kernels)} kernels, {sum(v[3] > 0 for v in kernels.values())} with private segment > 0, "
          f"{sum(v[0] == 512 for v in kernels.values())} at 512 VGPRs")


if __name__ == "__main__":
    main()
