"""csrc/ks_takeover.h on the host, without a GPU: the hand-over protocol of the rollout kernel's free-running waves (a wave that has done its
env-steps of a launch takes over half the envs of its workgroup's least-advanced wave).  tests/native/ks_takeover_host.cpp drives the header's
state machine - the code the kernel compiles - for four model waves on twelve plain words under a deterministic scheduler: every interleaving
of the first ticks (one tick = one access to the shared words, or one tick of an env-step), then seeded random schedules with random env-step
durations and deadlines that expire.  Start counts (4,4,4,4), (4,1,0,0), (2,0,0,0), (3,4,0,4); n_iter 1, 2, 3, 9.  In every schedule: every env is
stepped exactly n_iter times and in order, never by two waves in the same step; every wave terminates; a withdrawn request is never answered."""
import re
import subprocess
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
CSRC = HERE.parent / "kinovagrasping_amd" / "csrc"


@pytest.fixture(scope="module")
def program():
    exe, src = HERE / "native" / "ks_takeover_host", HERE / "native" / "ks_takeover_host.cpp"
    deps = [src, CSRC / "ks_takeover.h"]
    if not exe.exists() or any(d.stat().st_mtime > exe.stat().st_mtime for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", str(exe), str(src)])
    return exe


def _run(program, depth, n_random):
    r = subprocess.run([str(program), str(depth), str(n_random)], capture_output=True, text=True, timeout=300)
    print(r.stdout.strip())
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"ok: (\d+) schedules .* (\d+) grants taken \((\d+) from runs of two\), (\d+) declined, (\d+) expired waits", r.stdout)
    assert m, r.stdout
    return [int(g) for g in m.groups()]


def test_every_interleaving_of_the_first_ticks_keeps_the_step_count_exact(program):
    """4^8 schedule prefixes x 16 cases x (env-steps of 0 or 2 ticks) x (deadline never / 3 ticks), no random schedules: hand-overs, second
    splits, declined requests and expired waits all occur, and no schedule breaks an invariant."""
    runs, grants, from_pairs, declined, expired = _run(program, 8, 0)
    assert runs == 4 ** 8 * 16 * 4
    assert grants > 0 and from_pairs > 0 and declined > 0 and expired > 0


def test_random_schedules_with_random_durations_and_expiring_deadlines(program):
    """4000 seeded schedules per case: the wave to move is drawn at every tick, an env-step lasts 0 .. max_dur ticks (max_dur drawn per schedule,
    up to 40), every second schedule has a deadline of 1 .. 60 ticks"""
    runs, grants, from_pairs, declined, expired = _run(program, 0, 4000)
    assert runs == 16 * 4 + 16 * 4000                      # (depth 0: one round-robin schedule per variant)
    assert grants > runs // 4 and from_pairs > 0 and expired > 0
