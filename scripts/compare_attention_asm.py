#!/usr/bin/env python3
"""Do the existing attention kernels still have the code they had?  Cross-compiles csr5_attention.hip, csr5_attention_bwd.hip, the
two biased units (csr5_attention_bias.hip, csr5_attention_bwd_bias.hip), the two edge-biased ones (csr5_attention_edge.hip,
csr5_attention_bwd_edge.hip), the 16-bit ones (csr5_attention_lowp.hip, csr5_attention_bwd_lowp.hip) the additive-score ones
(csr5_attention_gat.hip, csr5_attention_bwd_gat.hip) and the dropped ones (csr5_attention_drop.hip, csr5_attention_drop_gat.hip,
csr5_attention_bwd_drop.hip, csr5_attention_bwd_drop_gat.hip, csr5_attention_drop_lowp.hip, csr5_attention_bwd_drop_lowp.hip) for gfx950 to assembly (hipcc -O3 --cuda-device-only
-S, once per value or operand type) from a git revision and from the working tree, and compares every kernel of the revision
(k_attention<..>, k_attention_bwd<..>, k_attention_biased<..>, k_attention_bwd_biased<..>, k_attention_edge<..>, k_attention_bwd_edge<..>, k_attention_lowp<..>, k_attention_bwd_lowp<..>, k_attention_gat<..>, k_attention_bwd_gat<..>) with the kernel of the same symbol
now, instruction for instruction and register for register.  No GPU needed.

    python scripts/compare_attention_asm.py [--rev HEAD~1] [--keep DIR]

The kernel templates are shared by the plain, the biased and the edge-biased entry points (csr5_attention_kern.h,
csr5_attention_bwd_kern.h, DESIGN.md sections 20 and 21), whose bodies are macros for exactly this property; run this after any
edit of those headers.  Exit status 0: every kernel of
the revision is identical in the working tree; 1: some differ (their names and the number of differing lines are printed) or are
missing.  Comment lines and trailing comments are ignored; nothing else is."""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("benchmark_spmv_using_csr5_amd", "csrc")
UNITS = (("csr5_attention.hip", "CSR5_ATTENTION_ONLY_F64"), ("csr5_attention.hip", "CSR5_ATTENTION_ONLY_F32"),
         ("csr5_attention_bwd.hip", "CSR5_ATTENTION_BWD_ONLY_F64"), ("csr5_attention_bwd.hip", "CSR5_ATTENTION_BWD_ONLY_F32"),
         ("csr5_attention_bias.hip", "CSR5_ATTENTION_ONLY_F64"), ("csr5_attention_bias.hip", "CSR5_ATTENTION_ONLY_F32"),
         ("csr5_attention_bwd_bias.hip", "CSR5_ATTENTION_BWD_ONLY_F64"), ("csr5_attention_bwd_bias.hip", "CSR5_ATTENTION_BWD_ONLY_F32"),
         ("csr5_attention_edge.hip", "CSR5_ATTENTION_ONLY_F64"), ("csr5_attention_edge.hip", "CSR5_ATTENTION_ONLY_F32"),
         ("csr5_attention_bwd_edge.hip", "CSR5_ATTENTION_BWD_ONLY_F64"), ("csr5_attention_bwd_edge.hip", "CSR5_ATTENTION_BWD_ONLY_F32"),
         ("csr5_attention_lowp.hip", "CSR5_LOWP_ONLY_BF16"), ("csr5_attention_lowp.hip", "CSR5_LOWP_ONLY_F16"),
         ("csr5_attention_bwd_lowp.hip", "CSR5_LOWP_ONLY_BF16"), ("csr5_attention_bwd_lowp.hip", "CSR5_LOWP_ONLY_F16"),
         ("csr5_attention_gat.hip", "CSR5_ATTENTION_ONLY_F64"), ("csr5_attention_gat.hip", "CSR5_ATTENTION_ONLY_F32"),
         ("csr5_attention_bwd_gat.hip", "CSR5_ATTENTION_BWD_ONLY_F64"), ("csr5_attention_bwd_gat.hip", "CSR5_ATTENTION_BWD_ONLY_F32"),
         ("csr5_attention_drop.hip", "CSR5_ATTENTION_ONLY_F64"), ("csr5_attention_drop.hip", "CSR5_ATTENTION_ONLY_F32"),
         ("csr5_attention_drop_gat.hip", "CSR5_ATTENTION_ONLY_F64"), ("csr5_attention_drop_gat.hip", "CSR5_ATTENTION_ONLY_F32"),
         ("csr5_attention_bwd_drop.hip", "CSR5_ATTENTION_BWD_ONLY_F64"), ("csr5_attention_bwd_drop.hip", "CSR5_ATTENTION_BWD_ONLY_F32"),
         ("csr5_attention_bwd_drop_gat.hip", "CSR5_ATTENTION_BWD_ONLY_F64"), ("csr5_attention_bwd_drop_gat.hip", "CSR5_ATTENTION_BWD_ONLY_F32"),
         ("csr5_attention_drop_lowp.hip", "CSR5_LOWP_ONLY_BF16"), ("csr5_attention_drop_lowp.hip", "CSR5_LOWP_ONLY_F16"),
         ("csr5_attention_bwd_drop_lowp.hip", "CSR5_LOWP_ONLY_BF16"), ("csr5_attention_bwd_drop_lowp.hip", "CSR5_LOWP_ONLY_F16"))


def kernels(tree, src, define, out):
    """symbol -> instruction lines of every kernel of one translation unit"""
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics",
           f"-I{os.path.join(tree, 'include')}", f"-D{define}", "--cuda-device-only", "-S", src, "-o", out]
    subprocess.run(cmd, cwd=os.path.join(tree, CSRC), check=True, stderr=subprocess.DEVNULL)
    found, cur = {}, None
    for line in open(out):
        line = re.sub(r";.*$", "", line).rstrip()
        m = re.match(r"^(_Z\w*k_attention\w*):$", line)
        if m:
            cur = found.setdefault(m.group(1), [])
        elif re.match(r"^\s*\.end_amdhsa_kernel|^\s*\.section", line):
            cur = None if ".section" in line else cur
        elif cur is not None and line.strip() and not re.match(r"^\s*\.(loc|file|ident)\b", line):
            cur.append(line)
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rev", default="HEAD~1", help="the revision whose kernels are the yardstick")
    ap.add_argument("--keep", default=None, help="keep the assembly files in this directory")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        work = args.keep or tmp
        os.makedirs(work, exist_ok=True)
        old = os.path.join(tmp, "rev")
        os.makedirs(old)
        tar = subprocess.run(["git", "-C", ROOT, "archive", args.rev, CSRC, "include"], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", old], input=tar, check=True)
        bad = total = 0
        for src, define in UNITS:
            if not os.path.exists(os.path.join(old, CSRC, src)):  # (a unit the revision does not have yet: nothing to compare)
                print(f"new unit  {src} ({define}): not in {args.rev}")
                continue
            tag = f"{os.path.splitext(src)[0]}_{define.rsplit('_', 1)[1].lower()}"  # (.._f64, .._f32, .._bf16, .._f16)
            was = kernels(old, src, define, os.path.join(work, f"rev_{tag}.s"))
            now = kernels(ROOT, src, define, os.path.join(work, f"tree_{tag}.s"))
            for name, text in was.items():
                total += 1
                if name not in now:
                    bad += 1
                    print(f"MISSING   {name}")
                elif now[name] != text:
                    bad += 1
                    lines = sum(1 for l in difflib.unified_diff(text, now[name], lineterm="", n=0) if l[:1] in "+-" and l[:3] not in ("+++", "---"))
                    print(f"DIFFERENT {name}: {lines} lines")
                else:
                    print(f"identical {name} ({len(text)} lines)")
        print(f"{total - bad} of {total} kernels of {args.rev} are identical in the working tree")
        return 1 if bad or not total else 0


if __name__ == "__main__":
    sys.exit(main())
