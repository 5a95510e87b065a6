"""Registers, LDS and scratch of the trunk and update-chain kernels, and what two resident trunk workgroups leave beside them.

Compiles serl_amd/csrc/trunk_f16x3.hip and heads.hip for gfx950 with hipcc's resource remarks (device code only: no link, no
GPU) and prints per kernel: VGPR + AGPR and their allocation (granule 8 of the 512 per lane per SIMD), LDS (static plus the dynamic
size its launcher passes), scratch, and what TWO resident workgroups of it (256 threads = one wave per SIMD each) leave over per
SIMD (registers) and per CU (of 160 KB LDS).  The update chain runs on a second stream beside the trunk pass of the next batch
(DESIGN.md sections 4 and 8): a chain workgroup that does not fit into that left-over starts only in a vacated trunk slot.

    python scripts/kernel_resources.py            # the table (flagship kernels first)
    python scripts/kernel_resources.py --all      # every kernel of the two files
    python scripts/kernel_resources.py --check    # exit 1 if a kernel of the two budget lists below exceeds its budget
"""
import argparse
import math
import os
import re
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "serl_amd", "csrc")
FILES = ("trunk_f16x3.hip", "heads.hip")
REGS_PER_SIMD, GRANULE, LDS_PER_CU = 512, 8, 160 * 1024

# Trunk launches of the flagship line (python bench.py: B = 256, 2 x 128x128, i.e. 1024 images per pass), in launch order:
# (kernel, launch, register budget, dynamic LDS bytes as an expression over the constexpr ints of csrc/*.h).  Two workgroups per CU.
RING_LDS = "4 * (128 * 64 + 64 * {tn} * 64)"     # trunk_f16x3.hip launch_dma: ring of four 16-channel slots
TRUNK = [
    ("conv_init_u8_kernel<2>", "conv_init", 216, "kC8Lds"),
    ("conv3x3_rowslab_f16x3_kernel", "b0_conv0", 216, "kRowslabLds"),
    ("conv3x3_slabdma_f16x3_kernel<true>", "b0_conv1, b1_conv1", 216, "kSlabDmaLds"),
    ("conv_dma_f16x3_kernel<2, 0, true>", "b1_conv0, b2_conv0 (+ projection)", 216, RING_LDS.format(tn=2)),
    ("conv_dma_f16x3_kernel<2, 0, false>", "b2_conv1", 216, RING_LDS.format(tn=2)),
    ("conv_dma_f16x3_kernel<2, 2, true>", "b3_conv0 (+ projection)", 216, RING_LDS.format(tn=2)),
    ("conv_dma_f16x3_kernel<2, 2, false>", "b3_conv1", 216, RING_LDS.format(tn=2)),
]
# Chain kernels of the flagship line (what a default critic step and actor step launch, profiles/chainfit_launches_*.txt): (kernel,
# budget = the smallest left-over per SIMD among the trunk launches it is meant to run beside).  80 = beside a 216-register trunk
# launch, i.e. everywhere; all of them are launched without dynamic LDS.
CHAIN = [
    ("sle_proprio_fwd_kernel<4, 2>", 80),
    ("sle_bwd_fused_kernel", 80),
    ("gemm_bf16x3_kernel<false, false, 16, false, false>", 80),
    ("gemm_bf16x3_kernel<true, false, 16, false, false>", 80),
    ("gemm_bf16x3_kernel<true, true, 16, false, false>", 80),
    ("ln_fwd_kernel<4, true>", 80),
    ("ln_bwd_kernel<0, false>", 80),
    ("ln_bwd_one_kernel<4, true>", 80),
    ("ln_bwd_one_kernel<1, false>", 80),
    ("ln_fwd_drop_kernel<4, true>", 80),      # the same rows with MLP Dropout (launches of a Dropout agent only)
    ("ln_bwd_drop_kernel<0, false>", 80),
    ("policy_dist_fwd_kernel<0>", 80),
    ("policy_dist_bwd_kernel<0>", 80),
    ("critic_loss_kernel", 80),
    ("colsum3_kernel", 80),
    ("adam_ema_kernel", 80),
    # read-only evaluation (serl_agent_eval_policy): launched on the update stream, possibly beside a prefetching trunk pass
    ("policy_stats_kernel<0>", 80),
    ("policy_stats_kernel<1>", 80),
    ("policy_stats_fixed_kernel<false>", 80),   # ... of a fixed-std agent (serl_agent_create_fixed_std)
    ("policy_stats_fixed_kernel<true>", 80),
]


def constants():
    """{name: value} of the `constexpr int k... = <expression>;` lines of csrc/*.h (expressions over earlier ones)"""
    found = {}
    for f in sorted(os.listdir(CSRC)):
        if f.endswith(".h"):
            for decl in re.finditer(r"constexpr\s+int\s+(k\w+\s*=[^;]+);", open(os.path.join(CSRC, f)).read()):
                for m in re.finditer(r"(k\w+)\s*=\s*([^,]+)", decl.group(1)):     # (one statement may declare several)
                    found[m.group(1)] = m.group(2)
    cache = {}

    def value(name):
        if name not in cache:
            expr = re.sub(r"//.*", "", found[name])
            cache[name] = int(eval(re.sub(r"\bk\w+\b", lambda m: str(value(m.group(0))), expr).replace("/", "//"), {"__builtins__": {}}))
        return cache[name]
    return value


def dynamic_lds(expr, value):
    return int(eval(re.sub(r"\bk\w+\b", lambda m: str(value(m.group(0))), expr), {"__builtins__": {}}))


def remarks(hipcc, src):
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-c", os.path.join(CSRC, src),
           "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if p.returncode:
        sys.stderr.write(p.stderr[-4000:])
        raise SystemExit(f"{src}: hipcc exited with {p.returncode}")
    kernels, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"remark:\s+([A-Za-z /\[\]]+?):\s+(\S+)\s+\[-Rpass-analysis", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            cur = kernels.setdefault(val, {})
        elif cur is not None:
            cur[key] = val
    return kernels


def demangle(names):
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not tool:
        return {n: n for n in names}
    out = subprocess.run([tool], input="\n".join(names), stdout=subprocess.PIPE, text=True).stdout.splitlines()
    short = {}
    for n, d in zip(names, out):
        d = re.sub(r"^void ", "", d).replace("serl::", "")
        depth, end = 0, len(d)
        for i, ch in enumerate(d):     # cut the parameter list, not the template arguments
            if ch == "<":
                depth += 1
            elif ch == ">":
                depth -= 1
            elif ch == "(" and depth == 0:
                end = i
                break
        short[n] = d[:end]
    return short


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--check", action="store_true", help="exit 1 if a kernel of the budget lists exceeds its budget (or is missing)")
    ap.add_argument("--all", action="store_true", help="list every kernel of the two files")
    args = ap.parse_args()
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        raise SystemExit("kernel_resources.py needs hipcc")
    with ThreadPoolExecutor(len(FILES)) as ex:
        per_file = list(ex.map(lambda f: remarks(hipcc, f), FILES))
    raw = {k: v for d in per_file for k, v in d.items()}
    short = demangle(list(raw))
    kern = {}
    for mangled, r in raw.items():
        regs = int(r["VGPRs"]) + int(r.get("AGPRs", 0))
        kern[short[mangled]] = {"regs": regs, "alloc": max(GRANULE, math.ceil(regs / GRANULE) * GRANULE),
                                "lds": int(r.get("LDS Size [bytes/block]", 0)), "scratch": int(r.get("ScratchSize [bytes/lane]", 0))}
    value = constants()
    bad = []
    head = f"{'kernel':52s} {'VGPR+AGPR':>9s} {'alloc':>5s} {'LDS st+dyn':>14s} {'scratch':>7s} {'left/SIMD':>9s} {'left LDS/CU':>11s}  "
    print("trunk launches, flagship path (two workgroups per CU; left = beside two of them)")
    print(head + "launch")
    left_min = REGS_PER_SIMD
    for name, launch, budget, dyn in TRUNK:
        k = kern.get(name)
        if k is None:
            bad.append(f"{name}: not compiled")
            continue
        d = dynamic_lds(dyn, value)
        left, left_lds = REGS_PER_SIMD - 2 * k["alloc"], LDS_PER_CU - 2 * (k["lds"] + d)
        left_min = min(left_min, left)
        print(f"{name:52s} {k['regs']:9d} {k['alloc']:5d} {k['lds']:6d}+{d:<7d} {k['scratch']:7d} {left:9d} {left_lds:11d}  {launch}")
        if k["alloc"] > budget or k["scratch"]:
            bad.append(f"{name}: {k['regs']} registers (allocation {k['alloc']}, budget {budget}), scratch {k['scratch']} (budget 0)")
    print(f"smallest left-over beside two trunk workgroups: {left_min} registers per lane per SIMD")
    print("\nupdate-chain kernels, flagship path (no dynamic LDS)")
    print(f"{'kernel':52s} {'VGPR+AGPR':>9s} {'alloc':>5s} {'LDS':>14s} {'scratch':>7s} {'budget':>9s}")
    for name, budget in CHAIN:
        k = kern.get(name)
        if k is None:
            bad.append(f"{name}: not compiled")
            continue
        print(f"{name:52s} {k['regs']:9d} {k['alloc']:5d} {k['lds']:14d} {k['scratch']:7d} {budget:9d}")
        if k["alloc"] > budget or k["scratch"]:
            bad.append(f"{name}: {k['regs']} registers (allocation {k['alloc']}) over its budget of {budget}, or scratch {k['scratch']}")
    if args.all:
        listed = {t[0] for t in TRUNK} | {c[0] for c in CHAIN}
        print("\nevery other kernel of " + ", ".join(FILES))
        print(f"{'kernel':52s} {'VGPR+AGPR':>9s} {'alloc':>5s} {'LDS static':>14s} {'scratch':>7s} {'left/SIMD':>9s}")
        for name in sorted(set(kern) - listed):
            k = kern[name]
            print(f"{name:52s} {k['regs']:9d} {k['alloc']:5d} {k['lds']:14d} {k['scratch']:7d} {REGS_PER_SIMD - 2 * k['alloc']:9d}")
    if bad:
        print("\nover budget:\n  " + "\n  ".join(bad))
    if args.check and bad:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
