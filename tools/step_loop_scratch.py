"""No GPU needed: resource lines and scratch-instruction counts inside the step loops of the role-specialised block filters, from
the device assembly of the filter3 family's translation unit -- the recipe of profiles/chain_carry_kernel_metadata.txt as a tool.

    hipcc <FLAGS of rpsmf_amd/build.py> -I include --save-temps --cuda-device-only -c rpsmf_amd/csrc/psmf_filter34.hip -o filter34_dev.o
    python tools/step_loop_scratch.py psmf_filter34-hip-amdgcn-amd-amdhsa-gfx950.s [kernel ...]

A step loop = a back-edge range (label ... branch back to it) that holds the 10 s_barrier of one step (up to 12 where a tail was
duplicated) and does not lie inside another such range; ranges that overlap (a rotated loop) count once.  The chain loop = the
smallest back-edge range that holds every step loop.  .private_segment_fixed_size = scratch bytes per lane.
digest = the first 16 hex digits of the SHA-256 of a step loop's instructions (comments, directives and label definitions dropped,
label operands replaced by one word): two builds whose digests agree run the same instructions on the same registers there."""

import hashlib
import re
import sys

KERNELS = ("psmf_blk_filter3", "psmf_blk_filter3s", "psmf_blk_filter4", "psmf_blk_filter5")
FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size",
          ".group_segment_fixed_size")


def kernel_body(lines, name):
    """(first, last) line index of the code of the kernel whose mangled name ends in `name` + 'ENS_11BlockParamsE'"""
    pat = re.compile(r"^(_ZN4psmf\d+" + re.escape(name) + r"ENS_11BlockParamsE):")
    for i, ln in enumerate(lines):
        m = pat.match(ln)
        if m:
            for j in range(i, len(lines)):
                if lines[j].startswith(".Lfunc_end"):
                    return m.group(1), i, j
    return None, -1, -1


def metadata(text, mangled):
    m = re.search(r"\.name:\s+" + re.escape(mangled) + r"\n", text)
    if m is None:
        return "(no metadata entry)"
    lo = text.rfind("  - .agpr_count:", 0, m.start())
    hi = text.find("  - .agpr_count:", m.end())
    block = text[lo:hi if hi > 0 else len(text)]
    return ", ".join(f + " " + re.search(re.escape(f) + r":\s*(\d+)", block).group(1) for f in FIELDS)


def count(lines, lo, hi, pat):
    return sum(1 for ln in lines[lo:hi + 1] if re.match(r"\s+" + pat, ln))


def digest(lines, lo, hi):
    body = []
    for ln in lines[lo:hi + 1]:
        ln = re.sub(r"\s*;.*$", "", ln).strip()
        if not ln or ln.startswith(".") or ln.endswith(":"):
            continue
        body.append(re.sub(r"\.LBB\d+_\d+", "L", ln))
    return hashlib.sha256("\n".join(body).encode()).hexdigest()[:16], len(body)


def main():
    path = sys.argv[1]
    names = sys.argv[2:] or KERNELS
    text = open(path).read()
    lines = text.split("\n")
    for name in names:
        mangled, a, b = kernel_body(lines, name)
        if mangled is None:
            print(f"{name}: not found")
            continue
        print(f"{name}: {metadata(text, mangled)}")
        label = {}
        ranges = []
        for i in range(a, b):
            m = re.match(r"^(\.LBB\d+_\d+):", lines[i])
            if m:
                label[m.group(1)] = i
            m = re.match(r"\s+s_c?branch\S*\s+(\.LBB\d+_\d+)", lines[i])
            if m and m.group(1) in label:
                ranges.append((label[m.group(1)], i))
        cand = [r for r in ranges if 10 <= count(lines, r[0], r[1], "s_barrier") <= 12]
        cand = [r for r in cand if not any(o != r and o[0] <= r[0] and r[1] <= o[1] for o in cand)]
        cand.sort()
        loops = []
        for r in cand:
            if loops and r[0] <= loops[-1][1]:
                loops[-1] = (loops[-1][0], max(loops[-1][1], r[1]))
            else:
                loops.append(r)
        outer = [r for r in ranges if loops and r[0] <= loops[0][0] and loops[-1][1] <= r[1] and r not in cand]
        chain = min(outer, key=lambda r: r[1] - r[0]) if outer else (a, b)
        print(f"  whole kernel: scratch_load {count(lines, a, b, 'scratch_load')}, scratch_store {count(lines, a, b, 'scratch_store')}, "
              f"{b - a} lines; chain loop [{chain[0] - a},{chain[1] - a}]")
        tl = ts = 0
        for n, (lo, hi) in enumerate(loops):
            f64, f32 = count(lines, lo, hi, "v_mfma_f64"), count(lines, lo, hi, "v_mfma_f32")
            sl, ss = count(lines, lo, hi, "scratch_load"), count(lines, lo, hi, "scratch_store")
            tl, ts = tl + sl, ts + ss
            dg, ni = digest(lines, lo, hi)
            print(f"  step loop {n} ({'inversion' if f64 else 'vector'} waves): lines [{lo - a},{hi - a}], s_barrier {count(lines, lo, hi, 's_barrier')}, "
                  f"v_mfma_f64 {f64}, v_mfma_f32 {f32}, scratch_load {sl}, scratch_store {ss}, instructions {ni}, digest {dg}")
        print(f"  inside the {len(loops)} step loops: scratch_load {tl}, scratch_store {ts}")


if __name__ == "__main__":
    main()
