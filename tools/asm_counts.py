#!/usr/bin/env python3
"""Instruction counts of the stepping kernels' gfx950 device assembly, per kernel / out-of-line function; diff of two trees.

    python tools/asm_counts.py                          # this tree, the kernels the solver is inlined into
    python tools/asm_counts.py --all                    # every function of ks_api.hip
    python tools/asm_counts.py --multi-geom             # the -DKS_MULTI_GEOM build
    python tools/asm_counts.py --against ../parent      # this tree against another checkout: per function the differences
    python tools/asm_counts.py --asm new.s --against-asm old.s   # the same on assembly that is already there

Needs hipcc only (cross-compiles, no GPU).  Per function: instructions, plain v_mov_b32, DPP moves (v_mov_b32_dpp), s_nop, the
floating-point arithmetic by mnemonic, registers (VGPR + AGPR) and scratch bytes.

The stepping kernels are one wave per SIMD: a lone wave pays per ISSUED instruction, so moves, waits and rows
nobody needs are time, and a change that removes only those must leave every floating-point count as it was - which mnemonic an
update got (v_fma_f32 or v_pk_mul_f32 + v_sub_f32) is its rounding.  The diff therefore COMPARES THE ARITHMETIC ONLY: it exits 1
if a floating-point count of any function differs, and reports everything else as a number.  Encodings are folded (_e32 / _e64 /
_dpp / _sdwa), so v_add_f32_dpp is a v_add_f32 and a v_mul_f32_dpp a v_mul_f32; a DPP multiply-add (v_fmac_f32_dpp: gfx9 has no
DPP form of v_fma_f32) is counted as the v_fma_f32 it replaces, not with the compiler's own v_fmac_f32."""
from __future__ import annotations

import argparse
import re
import shutil
import subprocess
import sys
import tempfile
from collections import Counter
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
DEFAULT_FILTER = r"k_env_step_f32|k_rollout<|k_substep<float|collision<float"
SUFFIX = re.compile(r"(_e32|_e64|_dpp|_sdwa)+$")
# floating-point arithmetic: anything that rounds (or selects by value) in fp32 / fp64 / packed fp32
FP = re.compile(r"^v_(pk_)?(fma|fmac|mad|mac|mul|add|sub|subrev|max|min|rcp|rsq|sqrt|div_scale|div_fmas|div_fixup|trig_preop|ldexp|"
                r"fract|floor|ceil|trunc|rndne|exp|log|sin|cos)(_legacy)?_f(32|64)$|^v_mfma_")
BEGIN = re.compile(r";\s*-- Begin function (\S+)")
RES = re.compile(r"^;\s*(NumVgprs|NumAgprs|ScratchSize):\s*(\d+)")
SHOWN = ["v_fma_f32", "v_fmac_f32", "v_pk_fma_f32", "v_pk_mul_f32", "v_mul_f32", "v_sub_f32", "v_add_f32"]


def hipcc() -> str:
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and Path(cand).exists():
            return cand
    sys.exit("asm_counts.py: hipcc not found")


def compile_asm(tree: Path, out: Path, multi_geom: bool, defines: list[str]) -> Path:
    csrc = tree / "kinovagrasping_amd" / "csrc"
    cmd = [hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-Wno-unused-command-line-argument"]
    cmd += (["-DKS_MULTI_GEOM"] if multi_geom else []) + [f"-D{d}" for d in defines] + ["-o", str(out), "ks_api.hip"]
    subprocess.check_call(cmd, cwd=str(csrc))
    return out


def demangle(names: list[str]) -> dict[str, str]:
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not filt or not names:
        return {n: n for n in names}
    out = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    short = {}
    for n, d in zip(names, out):
        d = d.replace("(anonymous namespace)::", "")
        d = d[5:] if d.startswith("void ") else d
        # name and template arguments, without the parameter list
        depth, end = 0, len(d)
        for i, ch in enumerate(d):
            if ch == "<":
                depth += 1
            elif ch == ">":
                depth -= 1
            elif ch == "(" and depth == 0:
                end = i
                break
        short[n] = d[:end]
    return short


def fold(mnemonic: str) -> str:
    """The operation an instruction performs, whatever its encoding."""
    if mnemonic.startswith("v_fmac_f32") and "_dpp" in mnemonic:
        return "v_fma_f32"
    return SUFFIX.sub("", mnemonic)


def count(path: Path) -> dict[str, dict]:
    """{mangled name: {"n": instructions, "mov": ..., "dpp_mov": ..., "nop": ..., "fp": Counter, "vgpr", "agpr", "scratch"}}"""
    fns: dict[str, dict] = {}
    cur = None          # the function whose body is being read
    last = None         # the function whose resource comments follow its body
    for line in path.read_text().splitlines():
        m = BEGIN.search(line)
        if m:
            cur = last = fns.setdefault(m.group(1), {"n": 0, "mov": 0, "dpp_mov": 0, "nop": 0, "fp": Counter(), "vgpr": 0, "agpr": 0, "scratch": 0})
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        r = RES.match(line)
        if r and last is not None:
            last[{"NumVgprs": "vgpr", "NumAgprs": "agpr", "ScratchSize": "scratch"}[r.group(1)]] = int(r.group(2))
            continue
        if cur is None or not line.startswith("\t"):
            continue
        word = line.split(None, 1)[0] if line.strip() else ""
        if not word or word[0] in ".;" or word.endswith(":"):
            continue
        cur["n"] += 1
        if word.startswith("v_mov_b32"):
            cur["dpp_mov" if "_dpp" in word else "mov"] += 1
        elif word == "s_nop":
            cur["nop"] += 1
        op = fold(word)
        if FP.match(op):
            cur["fp"][op] += 1
    return fns


def show(fns: dict[str, dict], names: dict[str, str], pat: re.Pattern | None) -> None:
    print(f"{'function':44s} {'instr':>7s} {'v_mov':>6s} {'dppmov':>6s} {'s_nop':>6s} " + " ".join(f"{s[2:-4]:>7s}" for s in SHOWN) + "  other-fp  vgpr+agpr  scratch")
    for n, c in fns.items():
        if pat and not pat.search(names[n]):
            continue
        other = sum(v for k, v in c["fp"].items() if k not in SHOWN)
        print(f"{names[n][:44]:44s} {c['n']:7d} {c['mov']:6d} {c['dpp_mov']:6d} {c['nop']:6d} " + " ".join(f"{c['fp'][s]:7d}" for s in SHOWN) +
              f"  {other:8d}  {c['vgpr']:4d}+{c['agpr']:<4d}  {c['scratch']:5d} B")


def diff(new: dict[str, dict], old: dict[str, dict], names: dict[str, str], pat: re.Pattern | None) -> int:
    bad = 0
    print(f"{'function':44s} {'instr':>15s} {'v_mov':>6s} {'dppmov':>6s} {'s_nop':>6s}  registers, scratch        floating-point arithmetic")
    for n in sorted(set(new) | set(old), key=lambda k: names.get(k, k)):
        if pat and not pat.search(names[n]):
            continue
        if n not in new or n not in old:
            print(f"{names[n][:44]:44s} only in the {'new' if n in new else 'old'} tree")
            bad += 1
            continue
        a, b = new[n], old[n]
        keys = sorted(set(a["fp"]) | set(b["fp"]))
        moved = [f"{k} {b['fp'][k]} -> {a['fp'][k]}" for k in keys if a["fp"][k] != b["fp"][k]]
        res = "same" if (a["vgpr"], a["agpr"], a["scratch"]) == (b["vgpr"], b["agpr"], b["scratch"]) else \
            f"{b['vgpr']}+{b['agpr']},{b['scratch']}B -> {a['vgpr']}+{a['agpr']},{a['scratch']}B"
        print(f"{names[n][:44]:44s} {b['n']:6d} ->{a['n']:6d} {a['mov'] - b['mov']:+6d} {a['dpp_mov'] - b['dpp_mov']:+6d} {a['nop'] - b['nop']:+6d}  {res:24s}  " +
              ("DIFFERS: " + ", ".join(moved) if moved else f"equal ({sum(a['fp'].values())} ops)"))
        bad += bool(moved)
    print("floating-point arithmetic: " + ("equal in every function listed" if not bad else f"{bad} function(s) differ"))
    return 1 if bad else 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--tree", type=Path, default=ROOT, help="checkout to compile (default: this one)")
    ap.add_argument("--against", type=Path, default=None, help="a second checkout: print the differences, exit 1 if any floating-point count differs")
    ap.add_argument("--asm", type=Path, default=None, help="read this assembly file instead of compiling --tree")
    ap.add_argument("--against-asm", type=Path, default=None, help="read this assembly file instead of compiling --against")
    ap.add_argument("--multi-geom", action="store_true", help="compile with -DKS_MULTI_GEOM")
    ap.add_argument("-D", dest="defines", action="append", default=[], help="further -D flags (e.g. KS_STAMP)")
    ap.add_argument("--filter", default=DEFAULT_FILTER, help="regular expression on the demangled name")
    ap.add_argument("--all", action="store_true", help="every function")
    ap.add_argument("--keep", type=Path, default=None, help="keep the assembly in this folder")
    args = ap.parse_args()
    pat = None if args.all else re.compile(args.filter)
    with tempfile.TemporaryDirectory() as tmp:
        out = args.keep or Path(tmp)
        out.mkdir(parents=True, exist_ok=True)
        tag = "_mg" if args.multi_geom else ""
        new = count(args.asm or compile_asm(args.tree, out / f"new{tag}.s", args.multi_geom, args.defines))
        old = None
        if args.against_asm or args.against:
            old = count(args.against_asm or compile_asm(args.against, out / f"old{tag}.s", args.multi_geom, args.defines))
    names = demangle(sorted(set(new) | set(old or {})))
    if old is None:
        show(new, names, pat)
        return 0
    return diff(new, old, names, pat)


if __name__ == "__main__":
    sys.exit(main())
