#!/usr/bin/env python3
"""Is a restructuring of the HIP sources neutral for the device code?  Compares, kernel by kernel, the gfx950 assembly of
two builds:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -save-temps=obj -c hip/UNIT.hip -o OLD/UNIT.o     (the old tree)
    ... the same for every translation unit of the new tree that now holds some of UNIT's kernels, into NEW/
    python tools/kernel_isa_diff.py OLD/UNIT-hip-amdgcn-amd-amdhsa-gfx950.s NEW/*-hip-amdgcn-amd-amdhsa-gfx950.s

Every kernel of the first file must be in exactly one of the others with the same instruction text and the same
.amdhsa_kernel block (registers, LDS, scratch), and the same resources in the metadata; the others may hold no kernel
the first has not.  Comments, debug / file directives and the per-function number in local labels are ignored.  Needs no
GPU.  Exit status 1 if anything differs."""
import re
import sys

META = ("vgpr_count", "sgpr_count", "agpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
        "vgpr_spill_count", "sgpr_spill_count", "max_flat_workgroup_size", "kernarg_segment_size")


def kernels(path):
    lines = open(path).read().split("\n")
    text, i = {}, 0
    while i < len(lines):
        m = re.match(r"^(_Z\w+):\s+; @", lines[i])
        if m and "@function" in lines[i - 1]:
            body = []
            i += 1
            while not lines[i].startswith(".Lfunc_end"):        # (the .amdhsa_kernel block lies inside this range)
                l = re.sub(r"\s*;.*$", "", lines[i]).rstrip()
                if l.strip() and not re.match(r"^\s*\.(loc|file|cfi_\w+)\b", l):
                    body.append(re.sub(r"\.LBB\d+_", ".LBB_", l))
                i += 1
            text[m.group(1)] = body
        i += 1
    whole = "\n".join(lines)
    meta = {}
    for ent in whole[whole.index("amdhsa.kernels:"):].split("\n  - .agpr_count:")[1:]:
        ent = ".agpr_count:" + ent
        meta[re.search(r"\.name:\s+(\S+)", ent).group(1)] = tuple(re.search(r"\.%s:\s+(\S+)" % k, ent).group(1) for k in META)
    return text, meta


def main():
    old, old_meta = kernels(sys.argv[1])
    new, new_meta, where = {}, {}, {}
    for p in sys.argv[2:]:
        t, m = kernels(p)
        for k in t:
            if k in new:
                sys.exit(f"{k} is in two of the new objects")
            new[k], new_meta[k], where[k] = t[k], m[k], p.split("/")[-1].split("-hip-")[0]
    bad = 0
    for k in sorted(old):
        if k not in new:
            print("missing:", k)
            bad += 1
        elif old[k] != new[k] or old_meta[k] != new_meta[k]:
            first = next((f"{a}  |  {b}" for a, b in zip(old[k], new[k]) if a != b), "(length or metadata)")
            print(f"differs: {k}: {old_meta[k]} / {new_meta[k]}; first difference: {first}")
            bad += 1
    extra = sorted(set(new) - set(old))
    for k in extra:
        print("only in the new objects:", k)
    by = {}
    for k in new:
        by[where[k]] = by.get(where[k], 0) + 1
    print(f"{len(old)} kernels before, {len(new)} after {by}; {sum(map(len, old.values()))} lines compared; "
          f"{bad} differ or are missing, {len(extra)} new")
    sys.exit(1 if bad or extra else 0)


if __name__ == "__main__":
    main()
