"""Instruction mix and register-hazard check of the exact-fp32 ring GEMM's k loop, read from the gfx950 assembly of csrc/gemm_bf16x3_v3.hip.

    python tools/kloop_isa.py                 # cross-compiles the two exact-fp32 instances (seconds, no GPU needed) and prints their mix
    python tools/kloop_isa.py --asm FILE.s    # the same on an assembly file that is already there

The k loop of an instance is found by its MFMAs: the basic blocks (label to label / branch) of the kernel that hold at least MIN_MFMAS matrix
instructions: two k-steps (the A fragments ping-pong) with an exit behind each, i.e. two blocks of 64 v_mfma_f32_16x16x4_f32.
Per block: the MFMA names, the other vector instructions by kind, scalar instructions, waits, and the reads in flight:
a `ds_read` destination is IN FLIGHT from its issue until an `s_waitcnt lgkmcnt(n)` with fewer younger LDS operations than n outstanding
retires it (LDS returns in order; the k loop issues no other lgkm operation in these blocks except scalar loads, which the check counts as
unordered and therefore as retiring nothing).  `hazards` lists every non-MFMA vector instruction that names an in-flight register.  A
k-step's last reads are retired by the next k-step's waits: the loop's blocks are analysed in the order they run, each starting with the reads
its predecessor left in flight (the last block's for the first).  `kernel_hazards` runs the check over every block of the kernel on its own.
tests/test_gemm_f32_kloop_isa_cpu.py asserts on the result."""
from __future__ import annotations

import argparse
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ladcast_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
MIN_MFMAS = 32
# mangled names: gemm_bf16x3_v3_kernel<128, 0, false> (the GEMM) and <128, 0, true> (the gathered conv, still on the 16x16x4 k-step)
KERNELS = {"gemm<128, 0, false>": "gemm_bf16x3_v3_kernelILi128ELi0ELb0EE", "conv<128, 0, true>": "gemm_bf16x3_v3_kernelILi128ELi0ELb1EE"}
MFMAS_PER_KSTEP = {"v_mfma_f32_16x16x4_f32": 64}


def compile_asm(out_dir, extra=()):
    """gemm_bf16x3_v3.hip -> gfx950 assembly (device side only)"""
    out = os.path.join(out_dir, "gemm_bf16x3_v3.s")
    # (LDC_GEMM_F32_INSTANCES_ONLY: the file's other twelve instances are not instantiated - seconds instead of minutes, the same code for these two)
    cmd = [HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only", "-S", "-DLDC_GEMM_F32_INSTANCES_ONLY", *extra,
           os.path.join(CSRC, "gemm_bf16x3_v3.hip"), "-o", out]
    subprocess.run(cmd, check=True, cwd=CSRC)
    return out


def kernel_body(asm, mangled):
    """the instruction lines of the one kernel whose symbol contains `mangled`"""
    lines = asm.splitlines()
    start = [i for i, ln in enumerate(lines) if re.match(r"^_Z\w*" + re.escape(mangled) + r"\w*:", ln)]
    assert len(start) == 1, (mangled, len(start))
    end = next(i for i in range(start[0], len(lines)) if lines[i].strip().startswith("s_endpgm"))
    return lines[start[0] + 1: end + 1]


def blocks_of(body):
    """basic blocks: a label starts one, a branch ends one"""
    out, cur = [], []
    for ln in body:
        t = ln.split(";")[0].strip()
        if not t or t.startswith("."):
            if re.match(r"^\.LBB\w+:", t) and cur:
                out.append(cur)
                cur = []
            continue
        cur.append(t)
        if t.startswith(("s_cbranch", "s_branch")):
            out.append(cur)
            cur = []
    if cur:
        out.append(cur)
    return out


def regs_of(operand):
    """vector registers an operand names: v12 -> {12}, v[8:11] -> {8..11}"""
    out = set()
    for m in re.finditer(r"\bv\[(\d+):(\d+)\]|\bv(\d+)\b", operand):
        if m.group(3) is not None:
            out.add(int(m.group(3)))
        else:
            out.update(range(int(m.group(1)), int(m.group(2)) + 1))
    return out


def analyse(block, entry=()):
    """entry: the reads in flight when the block starts, oldest first (as `in_flight` of the block that runs before it)"""
    mix = dict(mfma={}, ds_read=0, dma=0, valu={}, s_nop=0, salu=0, waits=0, barriers=0, hazards=[])
    in_flight = list(entry)  # (register set, text) of the reads in flight, oldest first
    for ins in block:
        op = ins.split()[0]
        args = ins[len(op):]
        if op.startswith("v_mfma"):
            mix["mfma"][op] = mix["mfma"].get(op, 0) + 1
            continue
        if op.startswith("ds_read"):
            mix["ds_read"] += 1
            in_flight.append((regs_of(args.split(",")[0]), ins))
            continue
        if op.startswith("global_load_lds") or (op.startswith(("global_load", "buffer_load")) and " lds" in ins):
            mix["dma"] += 1
        elif op == "s_waitcnt":
            mix["waits"] += 1
            m = re.search(r"lgkmcnt\((\d+)\)", ins)
            if m:
                keep = int(m.group(1))
                in_flight = in_flight[len(in_flight) - keep:] if keep < len(in_flight) else in_flight
                if keep == 0:
                    in_flight = []
        elif op == "s_barrier":
            mix["barriers"] += 1
        elif op == "s_nop":
            mix["s_nop"] += 1
        elif op.startswith("s_"):
            mix["salu"] += 1
        if op.startswith("v_") or op.startswith(("global_", "buffer_", "ds_write")):
            if op.startswith("v_"):
                kind = re.sub(r"_e(32|64)$", "", op)
                mix["valu"][kind] = mix["valu"].get(kind, 0) + 1
            named = regs_of(args)
            for regs, rd in in_flight:
                if named & regs:
                    mix["hazards"].append(f"{ins}   <- in flight: {rd}")
    mix["in_flight"] = in_flight
    return mix


def loop_blocks(asm, mangled):
    """[(k-steps in the block, mix)] of the kernel's loop blocks with MFMAs, and the same for its blocks without (a wave without rows)"""
    loop = [b for b in blocks_of(kernel_body(asm, mangled)) if sum(1 for i in b if i.startswith("v_mfma")) >= MIN_MFMAS]
    # the blocks run one after the other and the last one branches back to the first: a k-step's last reads are retired by the NEXT block's
    # waits, so each block is analysed with the reads its predecessor leaves in flight (one trip round the loop first, to get the first block's)
    entry = ()
    for b in loop:
        entry = analyse(b, entry)["in_flight"]
    out = []
    for b in loop:
        mix = analyse(b, entry)
        entry = mix["in_flight"]
        per = min(MFMAS_PER_KSTEP.get(k, 64) for k in mix["mfma"])
        out.append((sum(mix["mfma"].values()) / per, mix))
    return out


def kernel_hazards(asm, mangled):
    """the same register check over EVERY basic block of the kernel (the prologue's reads, the loop's exits, the epilogues)"""
    return [h for b in blocks_of(kernel_body(asm, mangled)) for h in analyse(b)["hazards"]]


def per_kstep(blocks):
    """summed over the loop's blocks and divided by their k-steps"""
    ks = sum(k for k, _ in blocks)
    tot = dict(mfma=0, ds_read=0, dma=0, valu=0, v_mov=0, s_nop=0, salu=0, waits=0, barriers=0)
    for _, m in blocks:
        tot["mfma"] += sum(m["mfma"].values())
        tot["valu"] += sum(m["valu"].values())
        tot["v_mov"] += sum(v for k, v in m["valu"].items() if k.startswith("v_mov") or k.startswith("v_accvgpr"))
        for k in ("ds_read", "dma", "s_nop", "salu", "waits", "barriers"):
            tot[k] += m[k]
    return {k: v / ks for k, v in tot.items()}, ks


def report(asm):
    for name, mangled in KERNELS.items():
        blocks = loop_blocks(asm, mangled)
        per, ks = per_kstep(blocks)
        names = sorted({k for _, m in blocks for k in m["mfma"]})
        kinds = {}
        for _, m in blocks:
            for k, v in m["valu"].items():
                kinds[k] = kinds.get(k, 0) + v
        print(f"{name}: {len(blocks)} loop block(s), {ks:g} k-step(s), {', '.join(names)}")
        print("  per wave and k-step: " + ", ".join(f"{k} {v:g}" for k, v in per.items()))
        print("  other vector instructions, all blocks: " + (", ".join(f"{k} {v}" for k, v in sorted(kinds.items())) or "none"))
        hz = [h for _, m in blocks for h in m["hazards"]]
        print(f"  vector instructions naming a register with a read in flight: {len(hz)}")
        for h in hz[:12]:
            print("    " + h)
        hz = kernel_hazards(asm, mangled)
        print(f"  the same over every block of the kernel: {len(hz)}")
        for h in hz[:12]:
            print("    " + h)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--asm", help="an assembly file of gemm_bf16x3_v3.hip for gfx950 (default: compile one)")
    a = ap.parse_args()
    if a.asm:
        report(open(a.asm).read())
    else:
        with tempfile.TemporaryDirectory() as d:
            report(open(compile_asm(d)).read())
