"""The hand-overs of the free-running rollout waves (csrc/ks_takeover.h: a wave that has done its env-steps of a launch takes over half the envs
of its workgroup's least-advanced wave): only WHO steps an env changes.  Per env the trajectory, the observations, the counters and the ring's
episodes stay those of the lock-step calls, bit for bit (tests.test_gpu_async._free_running_equals_lock_step).  n = 21, 22 and 277 CubeS envs
have a partly filled last group (5, 6 and 5 envs: waves with 1 or 2 envs, and waves with none that ask at once), so hand-overs are certain
there; among the full groups of n = 272 they may or may not happen."""
import pytest
import torch

from tests import test_gpu_async as ga

pytestmark = pytest.mark.gpu


def _equal_with_takeovers(monkeypatch, n, horizon, per):
    """the lock-step comparison, and the trainer's takeovers() of its five free-running launches"""
    from kinovagrasping_amd import pipeline
    seen = []

    class Recording(pipeline.AsyncTrainer):
        def counts(self):                       # (the comparison reads counts() once, after the last launch)
            seen.append(self.takeovers())
            return super().counts()

    monkeypatch.setattr(pipeline, "AsyncTrainer", Recording)
    ga._free_running_equals_lock_step((256, 256), False, horizon, per, n, expect_plan="waves")
    assert len(seen) == 1
    print(f"n={n} horizon={horizon} per={per}: takeovers (taken, expired, from runs of two) {seen[0]}")
    return seen[0]


@pytest.mark.parametrize("horizon,per", [(12, 9), (30, 13)])
@pytest.mark.parametrize("n", [21, 22, 277])
def test_hand_overs_leave_every_env_on_its_lock_step_trajectory(monkeypatch, n, horizon, per):
    taken, expired, from_pairs = _equal_with_takeovers(monkeypatch, n, horizon, per)
    assert taken > 0 and expired == 0
    if n == 21:                                 # the last group's waves hold 4, 1, 0, 0 envs: the second idle wave can only get a run split twice
        assert from_pairs > 0


@pytest.mark.parametrize("horizon,per", [(12, 9), (30, 13)])
@pytest.mark.parametrize("n", [21, 22, 277])
def test_switched_off_nothing_is_handed_over(monkeypatch, n, horizon, per):
    monkeypatch.setenv("KS_ROLLOUT_TAKEOVER", "0")
    assert _equal_with_takeovers(monkeypatch, n, horizon, per) == (0, 0, 0)


def test_full_groups_stay_equal_to_lock_step(monkeypatch):
    taken, expired, _ = _equal_with_takeovers(monkeypatch, 272, 30, 13)
    assert expired == 0
