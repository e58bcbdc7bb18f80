"""Register budget of the lean learner kernels beside the free-running rollout kernel (profiles/learner_400_300.txt).

A SIMD lane has 512 registers (VGPRs + AGPRs, one unified file on gfx950, allocated in granules of 8).  k_rollout holds its
allocation on every SIMD for a whole launch; a learner wave is resident beside it only when both allocations fit.  This reads
the compiler's resource remarks (-Rpass-analysis=kernel-resource-usage) for k_rollout<16,16>, k_rollout<25,19>, k_mlp3_lean<25,19>,
k_mlp3_bwd_lean<25,19> and the three observation-normalisation kernels of the learner's stream (k_obs_stats_update, k_obs_normalize,
k_fold_obs_norm), prints the table and exits non-zero when one of them beside k_rollout<25,19> exceeds 512 or uses scratch memory.

    python tools/learner_budget.py            # cross-compiles the two sources' device code (no GPU needed), nothing is installed
    python tools/learner_budget.py BUILD.log  # the captured output of kinovagrasping_amd.build.build(force=True, verbose=True)
"""
from __future__ import annotations

import re
import subprocess
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from kinovagrasping_amd import build as _build  # noqa: E402

FILE_REGS, GRANULE = 512, 8
KERNELS = {"k_rollout<16,16>": r"9k_rolloutILi16ELi16EE", "k_rollout<25,19>": r"9k_rolloutILi25ELi19EE",
           "k_mlp3_lean<25,19>": r"11k_mlp3_leanILi25ELi19EE", "k_mlp3_bwd_lean<25,19>": r"15k_mlp3_bwd_leanILi25ELi19EE",
           "k_obs_stats_update": r"18k_obs_stats_updateE", "k_obs_normalize": r"15k_obs_normalizeE", "k_fold_obs_norm": r"15k_fold_obs_normE"}
OBS_NORM = ("k_obs_stats_update", "k_obs_normalize", "k_fold_obs_norm")
PAIRINGS = [("k_rollout<25,19>", "k_mlp3_lean<25,19>"), ("k_rollout<25,19>", "k_mlp3_bwd_lean<25,19>")] + [("k_rollout<25,19>", k) for k in OBS_NORM]


def remarks() -> str:
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        for src in ("ks_api.hip", "ks_mlp.hip", "ks_rollout.hip"):
            cmd = [_build.hipcc_path(), "-Rpass-analysis=kernel-resource-usage", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                   "--cuda-device-only", "-c", "-o", str(Path(tmp) / (src + ".o")), str(_build.CSRC / src)]
            out.append(subprocess.run(cmd, cwd=str(_build.CSRC), check=True, stderr=subprocess.PIPE, text=True).stderr)
    return "\n".join(out)


def parse(text: str) -> dict:
    """{kernel: (vgpr, agpr, scratch bytes per lane)}; a kernel compiled more than once (the two libraries) keeps its largest figures"""
    found, name = {}, None
    for line in text.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = next((k for k, pat in KERNELS.items() if pat in m.group(1)), None)
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]): (\d+)", line)
        if m and name:
            key = {"VGPRs": 0, "AGPRs": 1}.get(m.group(1), 2)
            cur = found.setdefault(name, [0, 0, 0])
            cur[key] = max(cur[key], int(m.group(2)))
    return {k: tuple(v) for k, v in found.items()}


def allocation(vgpr: int, agpr: int) -> int:
    """registers the hardware sets aside per lane: the AGPRs start at the next multiple of 4, the total is rounded to the granule"""
    total = ((vgpr + 3) // 4 * 4 + agpr) if agpr else vgpr
    return (total + GRANULE - 1) // GRANULE * GRANULE


def main() -> int:
    res = parse(Path(sys.argv[1]).read_text() if len(sys.argv) > 1 else remarks())
    missing = [k for k in KERNELS if k not in res]
    if missing:
        print("no resource remark for: " + ", ".join(missing))
        return 2
    print(f"{'kernel':<26}{'VGPR':>6}{'AGPR':>6}{'allocated':>11}{'scratch B/lane':>16}{'left of 512':>13}")
    for k in KERNELS:
        v, a, s = res[k]
        print(f"{k:<26}{v:>6}{a:>6}{allocation(v, a):>11}{s:>16}{FILE_REGS - allocation(v, a):>13}")
    bad = 0
    for roll, lean in PAIRINGS:
        total = allocation(*res[roll][:2]) + allocation(*res[lean][:2])
        ok = total <= FILE_REGS and not (lean in OBS_NORM and res[lean][2])
        bad += not ok
        print(f"{roll} + {lean}: {total} of {FILE_REGS} -> {'resident together' if ok else 'DOES NOT FIT'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
