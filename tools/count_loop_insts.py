#!/usr/bin/env python3
"""Static instruction counts of the MFMA loops of a kernel, from the compiler's assembly (works without a GPU):

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt \
          -Iinclude -Igkgnet_amd/csrc --cuda-device-only -S gkgnet_amd/csrc/gkg_gemm_x6.hip -o x6.s
    python tools/count_loop_insts.py x6.s wgrad_x6_wide_kernel wgrad_x6_dma_kernel

For every backward branch of the kernel whose body holds MFMAs it prints the instructions between the branch target and the
branch, by class.  Blocks inside that range that are entered only through a forward branch (an edge tile's own code) are
counted in full, so a loop with such a block prints the sum of both paths; `--blocks` lists the range label by label.
"""
import collections
import re
import sys


def classify(op):
    if op.startswith("v_mfma"):
        return "MFMA"
    if op.startswith("v_accvgpr"):
        return "ACCMOV"
    if op.startswith(("scratch_", "buffer_store", "buffer_load")) and not op.endswith("lds"):
        return "VMEM"
    if op.startswith(("global_", "buffer_", "flat_")):
        return "VMEM"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith("s_waitcnt"):
        return "WAIT"
    if op.startswith("s_nop"):
        return "NOP"
    if op.startswith(("s_cbranch", "s_branch")):
        return "BRANCH"
    if op.startswith("s_"):
        return "SALU"
    if op.startswith("v_"):
        return "VALU"
    return "OTHER"


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    blocks = "--blocks" in sys.argv
    text = open(args[0]).read()
    for kern in args[1:]:
        m = re.search(r"^(_Z\w*?%d%s\w*):" % (len(kern), re.escape(kern)), text, re.M)     # the mangled name holds <length><name>
        if not m:
            print(kern, "not found")
            continue
        body = text[m.end():]
        body = body[:body.index(".end_amdhsa_kernel")] if ".end_amdhsa_kernel" in body else body
        lines = body[:body.index("s_endpgm")].splitlines() if "s_endpgm" in body else body.splitlines()
        label_at = {mm.group(1): i for i, l in enumerate(lines) for mm in [re.match(r"^(\.LBB\d+_\d+):", l)] if mm}
        insts = [(i, l.split()[0], l) for i, l in enumerate(lines)
                 if l.startswith("\t") and l.split() and not l.strip().startswith((".", ";"))]
        for i, op, l in insts:
            if not op.startswith(("s_cbranch", "s_branch")):
                continue
            tgt = l.split()[-1]
            if tgt not in label_at or label_at[tgt] > i:
                continue
            rng = [(j, o, ll) for j, o, ll in insts if label_at[tgt] < j <= i]
            c = collections.Counter(classify(o) for _, o, _ in rng)
            if not c["MFMA"]:
                continue
            ops = collections.Counter(o for _, o, _ in rng)
            valu = c["VALU"]
            print(f"{kern}: loop {tgt} .. line {i}: " + "  ".join(f"{k} {v}" for k, v in sorted(c.items()))
                  + f"  | VALU / MFMA {valu / c['MFMA']:.2f}")
            print("   " + "  ".join(f"{o} {n}" for o, n in sorted(ops.items()) if classify(o) in ("VALU", "ACCMOV", "SALU") and n >= 2))
            if blocks:
                cur, cc = tgt, collections.Counter()
                inner = sorted((v, k) for k, v in label_at.items() if label_at[tgt] <= v <= i)
                bounds = [v for v, _ in inner] + [i + 1]
                for (v, k), e in zip(inner, bounds[1:]):
                    cc = collections.Counter(classify(o) for j, o, _ in insts if v < j < e or j == e == i)
                    print(f"      {k}: " + "  ".join(f"{a} {b}" for a, b in sorted(cc.items())))


if __name__ == "__main__":
    main()
