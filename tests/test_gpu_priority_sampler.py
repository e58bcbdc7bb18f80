"""kr_commit_priorities, kr_sample_windows_prioritized and kr_update_priorities (csrc/ks_rollout.hip: k_commit_priorities, k_pick_prioritized,
k_gather_windows, k_update_priorities) through the C ABI against the plain loops of tests/priority_ref.py, between guard regions (the buffers
of tests/test_gpu_glue_kernels.py): which episode a batch slot takes, every gathered row and delta are pinned to the bit; the two powf
results - the importance weight and the quantised priority - to the allowance below.  Then prioritized replay end to end, in the lock-step
and in the free-running trainer."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

from kinovagrasping_amd import sim as ks
from tests import philox_ref
from tests import priority_ref as pr
from tests.test_gpu_glue_kernels import KS_ERR_INVALID, Buf, P, S, _lib, _rng, _stream, assert_bits, sent

pytestmark = pytest.mark.gpu

A = 4
OUT_ORDER = ("state", "action", "next", "reward", "not_done", "weight")
SENT_U32 = int(sent(1, np.uint32)[0])

# The device powf's error, in units of 2^-23 relative to the float64 value (one fp32 ulp at the top of a binade).  The ROCm installation the
# tests run on carries no table of the math functions' errors, so the figure is measured: the worst case over every powf result the tests of
# this file compare (691 comparisons: the importance weights of the row, long-table and trainer tests - each test prints its own worst case;
# the quantised priorities of the update tests are small enough for the floor's unit to cover them) was 0.843 units on an MI355X -
# profiles/prioritized_replay.txt -, and the allowance is twice that, rounded up to one decimal.
K_POWF = 1.7
ULP = 2.0 ** -23


def check_weights(got, ref, what):
    """the weight column against the reference's float64 power: zero where the reference is zero, else within K_POWF * 2^-23 relative"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    zero = ref == 0
    assert (got[zero] == 0).all(), f"{what}: a padding row has a weight"
    err = np.abs(got[~zero] - ref[~zero]) / (ULP * ref[~zero])
    worst = float(err.max()) if err.size else 0.0
    print(f"\nPRIO {what} | weight | worst powf error {worst:.3f} x 2^-23 over {err.size} rows")
    assert worst <= K_POWF, (what, worst)
    assert ((got[~zero] > 0) & (got[~zero] <= 1)).all(), what
    return worst


def check_entry(got, x_ref, what):
    """a table entry against the reference's float64 value x before the floor: off clamp(floor(x)) by at most 1 unit for the floor plus
    K_POWF * 2^-23 * x.  Returns what of the difference to x the floor cannot explain, in units of 2^-23 x (the powf error where x is large)."""
    want = float(pr.clamp_priority(x_ref))
    bound = 1.0 + K_POWF * ULP * want
    assert abs(float(got) - want) <= bound, (what, int(got), x_ref, bound)
    exact = min(max(x_ref, 1.0), float(pr.U32_MAX))
    return max(abs(float(got) - exact) - 1.0, 0.0) / (ULP * exact)


def upload(ring, offset=0):
    dev = {k: Buf(ring[k]) for k in pr.RING_FIELDS}
    dev.update(count=Buf(np.array([ring["count"]], np.int64)), head=Buf(np.array([ring["head"]], np.int64)), ep_len=Buf(ring["ep_len"]),
               ep_prio=Buf(np.concatenate([np.full(offset, 99, np.uint32), ring["ep_prio"]])))
    return dev


def kr_ring(ring, dev):
    return ks.KrRing(dev["count"].ptr, dev["head"].ptr, ring["capacity"], dev["ep_len"].ptr, dev["state"].ptr, dev["next"].ptr, dev["action"].ptr,
                     dev["reward"].ptr, dev["not_done"].ptr)


def outputs(batch, W, n):
    R = batch * W
    shapes = dict(state=(R, n, S), action=(R, n, A), next=(R, n, S), reward=(R, n), not_done=(R, n), weight=(R,))
    out = {k: Buf(sent(s, np.float32)) for k, s in shapes.items()}
    out["ends"], out["picked"] = Buf(sent((2 * R, S), np.float32)), Buf(sent(batch, np.int32))
    return out


def run_prioritized(batch, b_agent, H, n, agent, da, expert, de, beta, ue, us, draw, with_picked=True, seed=0, offset=0, with_ends=True):
    """one call with explicit uniforms (ue not None) or in-kernel draws; returns the output buffers"""
    out = outputs(batch, H - n, n)
    ra, re = kr_ring(agent, da), kr_ring(expert, de)
    keep = [Buf(ue), Buf(us)] if ue is not None else [None, None]
    dr = None if draw is None else Buf(np.array([draw], np.int64))
    bb = Buf(np.array([beta], np.float32))
    rc = _lib().kr_sample_windows_prioritized(batch, b_agent, H, n, ctypes.byref(ra), ctypes.byref(re), P(da["ep_prio"], 4 * offset), P(de["ep_prio"]),
                                              P(bb), P(keep[0]), P(keep[1]), seed, P(dr), *[P(out[k]) for k in OUT_ORDER],
                                              P(out["ends"]) if with_ends else None, P(out["picked"]) if with_picked else None, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert bb.unchanged() and all(k is None or k.unchanged() for k in keep)
    return out


def check(out, ref, what, with_picked=True):
    if with_picked:
        assert_bits(out["picked"].get(), ref[6], f"{what}: picked")
    else:
        assert out["picked"].unchanged()
    for k, want in zip(OUT_ORDER[:5], ref[:5]):
        assert_bits(out[k].get(), want, f"{what}: {k}")
    assert_bits(out["ends"].get(), ref[7], f"{what}: next_ends")
    return check_weights(out["weight"].get(), ref[5], what)


def philox_uniforms(index, tag, seed, draw):
    """the sampler's in-kernel uniforms: Philox4x32-10 at counter (index, draw low, draw high, tag), key (seed low, seed high); the first
    word's top 24 bits over 2^24"""
    index = np.asarray(index, np.uint64)
    full = lambda v: np.full_like(index, v)
    r = philox_ref.philox4x32_10((index, full(draw & 0xFFFFFFFF), full((draw >> 32) & 0xFFFFFFFF), full(tag)), (full(seed & 0xFFFFFFFF), full(seed >> 32)))
    return (r[0] >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


# ---- the commit -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("top", [3 * pr.PRIO_ONE + 5, 0, pr.U32_MAX])
@pytest.mark.parametrize("pattern", ["none", "all", "alternating"])
def test_commit_priorities(pattern, top):
    """test_commit_classes' set-up - 5 envs into a ring of 4 slots from head 3 (the slots wrap), rank from kr_rank_episodes -: the kept envs' slots
    get max(prio_max, 1), every other slot and the trash row keep the sentinel, prio_max itself is only read"""
    n, cap, head = 5, 4, 3
    keep = dict(none=np.zeros(n, np.uint8), all=np.array([1, 7, 1, 255, 1], np.uint8), alternating=np.array([1, 0, 1, 0, 1], np.uint8))[pattern]
    kb, rank, total = Buf(keep), Buf(sent(n, np.int64)), Buf(sent(1, np.int64))
    hb, tb, cb = Buf(np.array([head], np.int64)), Buf(np.array([top], np.uint32)), Buf(sent(cap + 1, np.uint32))
    L = _lib()
    assert L.kr_rank_episodes(n, P(kb), P(rank), P(total), _stream()) == 0
    assert L.kr_commit_priorities(n, cap, P(kb), P(rank), P(hb), P(tb), P(cb), _stream()) == 0
    want = pr.commit_priorities_ref(keep, rank.get(), head, cap, top, sent(cap + 1, np.uint32))
    assert_bits(cb.get(), want, "ep_prio")
    assert want[cap] == SENT_U32 and int((want[:cap] == max(top, 1)).sum()) == {"none": 0, "all": 4, "alternating": 3}[pattern]
    assert kb.unchanged() and hb.unchanged() and tb.unchanged()


# ---- pick and gather, every row ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count,head", pr.COUNT_HEAD)
def test_prioritized_sampler_every_row(count, head):
    """horizon 8, n_steps 3 (W = 5), 6 batch slots, an agent ring of 8 slots at every (count, head) of the CPU test's list and an expert ring of 5;
    tables of equal priorities, of 1 and 2^32 - 1 side by side with a stored 0, random ones; uniforms on 0, on 1 - 2^-24 and on and beside the
    prefix-sum boundaries, and Philox draws; batch_agent 0, 4 and 6; with and without `picked` and next_ends: picked, every output row - the
    weight-0 rows too - and next_ends equal priority_ref bit for bit, the weights within the powf allowance"""
    H, n, W = pr.H, pr.N_STEPS, pr.H - pr.N_STEPS
    worst = 0.0
    for name in ("equal", "extremes", "random", "near_one"):
        r = _rng("prio rows", count, head, name)
        agent = pr.make_ring(pr.CAP, H, count, head, pr.ring_lens(H, n), pr.priority_patterns(pr.CAP, r)[name], r)
        expert = pr.make_ring(5, H, 4, 2, [n + 2, H, n + 1, H, n + 3], [3 * pr.PRIO_ONE, 1, pr.PRIO_ONE // 7, pr.U32_MAX, 5], r)
        da, de = upload(agent), upload(expert)
        for shift, beta in enumerate((1.0, 0.4, 0.0)):
            ue = pr.episode_uniforms(pr.B, agent, shift)
            ue[pr.B_AGENT:] = pr.episode_uniforms(pr.B - pr.B_AGENT, expert, shift)
            us = pr.start_uniforms(pr.B, W, shift)
            what = f"{name} beta {beta}"
            out = run_prioritized(pr.B, pr.B, H, n, agent, da, agent, da, beta, ue, us, None)
            worst = max(worst, check(out, pr.sample_prioritized_ref(pr.B, H, n, agent, ue, us, beta), what + " one ring"))
            for b_agent in ((0, pr.B_AGENT, pr.B) if shift == 0 else (pr.B_AGENT,)):
                with_picked = b_agent != pr.B_AGENT or shift == 1
                out = run_prioritized(pr.B, b_agent, H, n, agent, da, expert, de, beta, ue, us, None, with_picked=with_picked)
                ref = pr.sample_prioritized_ref(pr.B, H, n, agent, ue, us, beta, expert=expert, batch_agent=b_agent)
                worst = max(worst, check(out, ref, what + f" batch_agent {b_agent}", with_picked))
        # in-kernel draws: the uniforms are Philox's, the batch the reference's on those
        seed, draw = 0x1234567890ABCDEF, 2 ** 40 + 77
        ue, us = philox_uniforms(np.arange(pr.B), 0x5a4d, seed, draw), philox_uniforms(np.arange(pr.B * W), 0x5a4e, seed, draw).reshape(pr.B, W)
        for with_picked in (True, False):
            out = run_prioritized(pr.B, pr.B_AGENT, H, n, agent, da, expert, de, 0.6, None, None, draw, seed=seed, with_picked=with_picked)
            ref = pr.sample_prioritized_ref(pr.B, H, n, agent, ue, us, 0.6, expert=expert, batch_agent=pr.B_AGENT)
            worst = max(worst, check(out, ref, f"{name} philox", with_picked))
        assert all(b.unchanged() for b in list(da.values()) + list(de.values()))
    print(f"\nPRIO rows count {count} head {head} | worst powf error {worst:.3f} x 2^-23")


# ---- long tables: the pick alone, through `picked` ---------------------------------------------------------------------------------------
ELIGIBLE = (1, 2, 255, 256, 257, 1535, 1536, 1537, 2047, 2048, 2049, 4100)


@pytest.mark.parametrize("wrapped", [False, True], ids=["unwrapped", "wrapped"])
@pytest.mark.parametrize("eligible", ELIGIBLE)
def test_prioritized_pick_on_long_tables(eligible, wrapped):
    """eligible counts around one trip of the table walk (256 priorities), around one group of trips (1536: what the walk keeps in flight) and
    around 2048, and 4100 (several groups, the last one partial); the eligible range in one piece (head = count) or wrapped into two with ragged
    ends (a full ring, head mid-table); the table 0 - 3 elements behind a 16-byte boundary; priorities all 1, all 2^32 - 1, random, and 1 with
    a few 2^32 - 1; uniforms 0, 1 - 2^-24, values at and beside prefix-sum boundaries and random ones.  W = 1; compared through `picked`: exact."""
    H, n, batch = 4, 3, 24
    if wrapped:
        cap = count = eligible + 1
        head = (2 * cap) // 3 if cap > 2 else 1
    else:
        cap, count = eligible + 3, eligible + 1
        head = count
    r = _rng("long prio", eligible, wrapped)
    zeros = {f: np.zeros(s, np.float32) for f, s in dict(state=(cap, H, S), next=(cap, H, S), action=(cap, H, A), reward=(cap, H), not_done=(cap, H)).items()}
    tables = {"ones": np.ones(cap, np.uint32), "max": np.full(cap, pr.U32_MAX, np.uint32),
              "random": r.randint(0, 2 ** 32, cap, dtype=np.uint64).astype(np.uint32),
              "spikes": np.where(r.rand(cap) < 0.01, pr.U32_MAX, 1).astype(np.uint32)}
    for offset, (name, table) in zip((0, 1, 2, 3), tables.items()):
        for off in sorted({offset, (offset + 2) % 4}):
            ring = dict(count=count, head=head, capacity=cap, ep_len=np.full(cap, H, np.int64), ep_prio=table, **zeros)
            dev = upload(ring, offset=off)
            elig = pr.eligible_priorities(ring)
            assert len(elig) == eligible
            total = sum(p for _, p in elig)
            bounds = np.cumsum([p for _, p in elig], dtype=np.float64)[r.randint(0, eligible, 6)] / total
            ue = np.concatenate([[0.0, pr.TOP, 0.5], bounds, np.nextafter(bounds.astype(np.float32), np.float32(0)), r.rand(batch)]).astype(np.float32)
            ue = ue[(ue >= 0) & (ue < 1)][:batch]
            assert len(ue) == batch
            out = run_prioritized(batch, batch, H, n, ring, dev, ring, dev, 0.5, ue, np.zeros((batch, 1), np.float32), None, offset=off, with_ends=False)
            picks = pr.pick_ref(ring, batch, ue, 0.5)
            assert_bits(out["picked"].get(), np.asarray([p[0] for p in picks], np.int32), f"{name} offset {off}: picked")
            check_weights(out["weight"].get(), [p[1] for p in picks], f"eligible {eligible} {name} offset {off}")
            assert dev["ep_prio"].unchanged()
            if eligible > 1:
                assert len({p[0] for p in picks}) > 1 and all(p[0] != (head - 1) % cap for p in picks)


# ---- the update -------------------------------------------------------------------------------------------------------------------------
def update_case(r, order=(0, 1, 2, 3, 4, 5)):
    """6 batch episodes x 5 rows, 4 agent + 2 expert.  Agent: episodes 0 and 3 were read from the same slot (3), episode 1 has no real row,
    episode 2 a NaN q on a real row; expert: both episodes from slot 1, the second with an infinite q.  `order` permutes the batch episodes
    within their segments (rows, picked) - the tables must not depend on it."""
    batch, b_agent, W, n = 6, 4, 5, 3
    R = batch * W
    q, tq1 = (r.standard_normal(R) * 3).astype(np.float32), (r.standard_normal(R) * 3).astype(np.float32)
    reward = (r.rand(R, n) * 5).astype(np.float32)
    weight = (0.05 + 0.95 * r.rand(R)).astype(np.float32)
    weight[[4, 14, 19, 28, 29]] = 0                        # padding rows
    weight[5:10] = 0                                        # episode 1: no real row
    q[11] = np.nan                                          # episode 2, a real row
    q[13] = 1e30
    q[14] = np.nan                                          # (a padding row: ignored)
    q[26] = np.inf                                          # episode 5
    picked = np.array([3, 5, 2, 3, 1, 1], np.int32)
    rows = np.concatenate([np.arange(b * W, (b + 1) * W) for b in order])
    return batch, b_agent, W, n, q[rows], tq1[rows], reward[rows], weight[rows], picked[list(order)]


def run_update(case, alpha, eps_a, eps_e, tops=(pr.PRIO_ONE, 2 ** 31 + 5), with_delta=True, discount=0.995):
    batch, b_agent, W, n, q, tq1, reward, weight, picked = case
    bufs = dict(q=Buf(q), tq1=Buf(tq1), reward=Buf(reward), weight=Buf(weight), picked=Buf(picked))
    tabs = dict(agent=Buf(sent(7 + 1, np.uint32)), expert=Buf(sent(5 + 1, np.uint32)), agent_max=Buf(np.array([tops[0]], np.uint32)),
                expert_max=Buf(np.array([tops[1]], np.uint32)), delta=Buf(sent(batch, np.float32)))
    rc = _lib().kr_update_priorities(batch, b_agent, W + n, n, P(bufs["q"]), P(bufs["tq1"]), P(bufs["reward"]), P(bufs["weight"]), discount, P(bufs["picked"]),
                                     alpha, eps_a, eps_e, P(tabs["agent"]), P(tabs["expert"]), P(tabs["agent_max"]), P(tabs["expert_max"]),
                                     P(tabs["delta"]) if with_delta else None, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert all(b.unchanged() for b in bufs.values())
    return tabs


@pytest.mark.parametrize("alpha,eps_a,eps_e", [(0.3, 1e-3, 1.0), (1.0, 0.0, 0.5), (0.0, 1e-3, 1.0), (2.5, 3.0, 1e4)])
def test_update_priorities(alpha, eps_a, eps_e):
    """delta_out equals the float32 reference in every bit (-1 without a real row, NaN and inf where they are); the table entries of the picked
    slots are the quantised maxima within the powf allowance (alpha 2.5 with eps 1e4 saturates at 2^32 - 1, alpha 0 gives exactly 65536); the
    slot of an episode without a real row and the one with a NaN stay the sentinel, as every slot nobody picked and the trash rows; the
    expert segment uses eps_expert and its own table and prio_max; each prio_max is the maximum of its old value and what was written; no
    input changes; and with the duplicates' batch order permuted the tables and maxima are the same in every bit"""
    r = _rng("update", alpha)
    case = update_case(r)
    batch, b_agent, W, n, q, tq1, reward, weight, picked = case
    tabs = run_update(case, alpha, eps_a, eps_e)
    deltas, written = pr.update_priorities_ref(batch, b_agent, W, n, q, tq1, reward, weight, 0.995, picked, alpha, eps_a, eps_e)
    got_delta = tabs["delta"].get()
    assert got_delta.view(np.uint32).tolist() == deltas.view(np.uint32).tolist(), (got_delta, deltas)
    assert deltas[1] == -1 and np.isnan(deltas[2]) and np.isinf(deltas[5]) and np.isfinite(deltas[[0, 3, 4]]).all()
    assert sorted(written[0]) == [3] and sorted(written[1]) == [1]
    worst = 0.0
    for seg, name, top in ((0, "agent", pr.PRIO_ONE), (1, "expert", 2 ** 31 + 5)):
        table = tabs[name].get()
        for s in range(len(table)):
            if s in written[seg]:
                worst = max(worst, check_entry(table[s], written[seg][s], f"{name} slot {s}"))
            else:
                assert table[s] == SENT_U32, (name, s, table[s])
        assert int(tabs[name + "_max"].get()[0]) == max([top] + [int(table[s]) for s in written[seg]])
    if alpha == 0.0:
        assert int(tabs["agent"].get()[3]) == pr.PRIO_ONE and int(tabs["expert"].get()[1]) == pr.PRIO_ONE
    if alpha == 2.5:
        assert int(tabs["expert"].get()[1]) == pr.U32_MAX and int(tabs["expert_max"].get()[0]) == pr.U32_MAX
    print(f"\nPRIO update alpha {alpha} | worst powf error on a table entry {worst:.3f} x 2^-23")
    assert worst <= K_POWF
    # the duplicates in the other batch order, and the whole segments reversed
    for order in ((3, 1, 2, 0, 5, 4), (3, 2, 1, 0, 5, 4), (0, 3, 1, 2, 4, 5)):
        other = run_update(update_case(_rng("update", alpha), order), alpha, eps_a, eps_e, with_delta=order[0] == 0)
        for k in ("agent", "expert", "agent_max", "expert_max"):
            assert other[k].get().tobytes() == tabs[k].get().tobytes(), (order, k)
        if order[0] != 0:
            assert other["delta"].unchanged()


def test_update_priorities_takes_the_maximum_of_duplicates_whichever_comes_first():
    """the same slot read by three agent episodes whose deltas are 0.25, 4 and 1 (q = 0, reward = 0, tq1 chosen; discount 1; exact in fp32): with
    alpha 1 and eps 0 the entry is 4 * 65536 (within the allowance) and the same value in all six batch orders, and prio_max follows"""
    seen = set()
    W, n = 2, 1
    for order in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
        deltas = np.array([0.25, 4.0, 1.0], np.float32)[list(order)]
        tq1 = np.repeat(deltas, W) * np.tile(np.array([1.0, 0.5], np.float32), 3)
        case = (3, 3, W, n, np.zeros(6, np.float32), tq1.astype(np.float32), np.zeros((6, n), np.float32), np.ones(6, np.float32), np.array([6, 6, 6], np.int32))
        tabs = run_update(case, 1.0, 0.0, 0.0, discount=1.0)
        assert tabs["delta"].get()[:3].tolist() == deltas.tolist()
        table = tabs["agent"].get()
        check_entry(table[6], 4.0 * pr.PRIO_ONE, f"order {order}")
        assert (np.delete(table, 6) == SENT_U32).all(), (order, table)
        assert int(tabs["agent_max"].get()[0]) == int(table[6]) and tabs["expert"].unchanged() and tabs["expert_max"].unchanged()
        seen.add(int(table[6]))
    assert len(seen) == 1


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def _valid_sample_call():
    H, ns, cap, W = 8, 5, 4, 3
    fz = lambda *s: Buf(np.zeros(s, np.float32))
    rings = []
    for _ in range(2):
        rings.append(dict(count=Buf(np.array([3], np.int64)), head=Buf(np.array([3], np.int64)), capacity=cap, ep_len=Buf(np.full(cap, H, np.int64)),
                          ep_state=fz(cap, H, S), ep_next=fz(cap, H, S), ep_action=fz(cap, H, A), ep_reward=fz(cap, H), ep_not_done=fz(cap, H)))
    R = 2 * W
    table = lambda: Buf(np.array([5, 1, 70000, 9], np.uint32))
    return [2, 1, H, ns, rings[0], rings[1], table(), table(), Buf(np.array([0.5], np.float32)), fz(2), fz(2, W), 5, Buf(np.array([2], np.int64)),
            fz(R, ns, S), fz(R, ns, A), fz(R, ns, S), fz(R, ns), fz(R, ns), fz(R), fz(2 * R, S), Buf(np.zeros(2, np.int32))]


SAMPLE_REFUSALS = [("batch 0", 0, 0), ("batch_agent > batch", 1, 3), ("batch_agent -1", 1, -1), ("horizon == n_steps", 2, 5), ("n_steps 65", (2, 3), (70, 65)),
                   ("n_steps 0", 3, 0), ("agent ring NULL", 4, None), ("expert ring NULL", 5, None), ("agent_prio NULL", 6, None),
                   ("expert_prio NULL", 7, None), ("beta NULL", 8, None), ("u_ep without u_start", 10, None), ("u_start without u_ep", 9, None),
                   ("no uniforms and no draw", (9, 10, 12), None)] + \
                  [(f"NULL output {k}", k, None) for k in range(13, 19)] + \
                  [(f"{which} ring without {f}", (4 if which == "agent" else 5, f), None) for which in ("agent", "expert")
                   for f in ("count", "head", "ep_len", "ep_state", "ep_next", "ep_action", "ep_reward", "ep_not_done", "capacity")] + \
                  [(f"{which} capacity above 2^20", (4 if which == "agent" else 5, "capacity"), 2 ** 20 + 1) for which in ("agent", "expert")]


def _call(fn, args):
    keep_alive = []

    def conv(a):
        if isinstance(a, dict):
            g = ks.KrRing(*[(a[k].ptr if isinstance(a[k], Buf) else a[k]) for k in ("count", "head", "capacity", "ep_len", "ep_state", "ep_next", "ep_action",
                                                                                      "ep_reward", "ep_not_done")])
            keep_alive.append(g)
            return ctypes.byref(g)
        return P(a) if isinstance(a, Buf) else a
    return getattr(_lib(), fn)(*[conv(a) for a in args], _stream())


def _refuse(fn, args, rings, label, index, value):
    bufs = [a for a in args if isinstance(a, Buf)] + [b for g in rings for b in g.values() if isinstance(b, Buf)]
    if isinstance(index, tuple) and isinstance(index[1], str):
        args[index[0]] = dict(args[index[0]])
        args[index[0]][index[1]] = value if value is not None else (0 if index[1] == "capacity" else None)
    else:
        for j, k in enumerate(index if isinstance(index, tuple) else (index,)):
            args[k] = value[j] if isinstance(value, tuple) else value
    assert _call(fn, args) == KS_ERR_INVALID, label
    torch.cuda.synchronize()
    assert all(b.unchanged() for b in bufs), label


@pytest.mark.parametrize("label,index,value", SAMPLE_REFUSALS, ids=[c[0].replace(" ", "_") for c in SAMPLE_REFUSALS])
def test_prioritized_sampler_refusals(label, index, value):
    """what kr_sample_windows_mixed refuses, a NULL beta, and for a ring that has batch slots a NULL priority table or a capacity above 2^20:
    KS_ERR_INVALID, and no buffer of the call has changed"""
    args = _valid_sample_call()
    _refuse("kr_sample_windows_prioritized", args, args[4:6], label, index, value)


def _valid_update_call():
    batch, W, n = 2, 3, 5
    R = batch * W
    fz = lambda *s: Buf(np.zeros(s, np.float32))
    table = lambda: Buf(np.array([5, 1, 70000, 9], np.uint32))
    top = lambda: Buf(np.array([pr.PRIO_ONE], np.uint32))
    return [batch, 1, W + n, n, fz(R), fz(R), fz(R, n), Buf(np.ones(R, np.float32)), 0.99, Buf(np.array([1, 2], np.int32)), 0.3, 1e-3, 1.0, table(), table(),
            top(), top(), fz(batch)]


UPDATE_REFUSALS = [("batch 0", 0, 0), ("batch_agent > batch", 1, 3), ("batch_agent -1", 1, -1), ("horizon == n_steps", 2, 5), ("n_steps 0", 3, 0),
                   ("q NULL", 4, None), ("tq1 NULL", 5, None), ("reward NULL", 6, None), ("weight NULL", 7, None), ("discount NaN", 8, float("nan")),
                   ("picked NULL", 9, None), ("alpha negative", 10, -0.5), ("alpha NaN", 10, float("nan")), ("eps_agent negative", 11, -1e-3),
                   ("eps_expert NaN", 12, float("nan")), ("agent_prio NULL", 13, None), ("expert_prio NULL", 14, None), ("agent_prio_max NULL", 15, None),
                   ("expert_prio_max NULL", 16, None)]


@pytest.mark.parametrize("label,index,value", UPDATE_REFUSALS, ids=[c[0].replace(" ", "_") for c in UPDATE_REFUSALS])
def test_update_priorities_refusals(label, index, value):
    """one case per argument of kr_update_priorities: KS_ERR_INVALID, and no buffer of the call has changed"""
    args = _valid_update_call()
    _refuse("kr_update_priorities", args, [], label, index, value)


def test_the_valid_calls_and_their_optional_arguments():
    """the refusal lists' calls run; so they do without next_ends, picked and delta_out, and with a NULL table (and prio_max) for a ring that has
    no batch slots; kr_commit_priorities refuses n = 0, capacity = 0 and each NULL pointer"""
    for change in ({}, {19: None, 20: None}, {1: 2, 7: None}, {1: 0, 6: None}):
        args = _valid_sample_call()
        for k, v in change.items():
            args[k] = v
        assert _call("kr_sample_windows_prioritized", args) == 0, change
    for change in ({}, {17: None}, {1: 2, 14: None, 16: None}, {1: 0, 13: None, 15: None}):
        args = _valid_update_call()
        for k, v in change.items():
            args[k] = v
        assert _call("kr_update_priorities", args) == 0, change
    torch.cuda.synchronize()
    commit = lambda: [3, 4, Buf(np.ones(3, np.uint8)), Buf(np.array([1, 2, 3], np.int64)), Buf(np.array([0], np.int64)), Buf(np.array([7], np.uint32)),
                      Buf(np.zeros(5, np.uint32))]
    assert _call("kr_commit_priorities", commit()) == 0
    for k, v in [(0, 0), (1, 0)] + [(k, None) for k in range(2, 7)]:
        args = commit()
        args[k] = v
        assert _call("kr_commit_priorities", args) == KS_ERR_INVALID, k
        torch.cuda.synchronize()
        assert all(a.unchanged() for a in args if isinstance(a, Buf))


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def _setup(n=64, horizon=12):
    from kinovagrasping_amd import scenarios
    from kinovagrasping_amd.ddpgfd import DDPGfD
    from kinovagrasping_amd.multi_shape import MultiShapeSim
    from kinovagrasping_amd.replay import DeviceEpisodeReplay
    from kinovagrasping_amd.rollout import RolloutEngine
    rng = np.random.RandomState(4)
    sim = MultiShapeSim(n, ["CubeS"], device=0, auto_reset=True, horizon=horizon)
    qp, hqp, _ = scenarios.draw_start_pool(["CubeS"] * n, "normal", 4, rng)
    sim.reset(torch.as_tensor(qp[0]), torch.as_tensor(hqp[0]), object_id=sim.shape_of_env)
    obs0 = sim.set_start_pool(torch.as_tensor(qp), torch.as_tensor(hqp), seed=2)
    torch.manual_seed(2)
    policy = DDPGfD(82, 4, 0.8, 5, batch_size=8, hidden=(64, 64), device=sim.device)
    replay = DeviceEpisodeReplay(n, capacity=8 * n, horizon=horizon, device=sim.device)
    eng = RolloutEngine(sim, policy, replay, expl_noise=0.1)
    eng.start(obs0)
    return sim, policy, replay, eng


def _host_ring(replay, table):
    cap = replay.capacity
    g = lambda t: t[:cap].cpu().numpy()
    return dict(count=replay.count, head=replay.head, capacity=cap, ep_len=g(replay.ep_len), ep_prio=np.asarray(table[:cap], np.uint32), state=g(replay.ep_state),
                next=g(replay.ep_next), action=g(replay.ep_action), reward=g(replay.ep_reward), not_done=g(replay.ep_not_done))


def test_lock_step_trainer_samples_by_priority_and_writes_the_errors_back():
    """GraphedTrainer(prioritized=True), 64 envs, CubeS, horizon 12, eager: the ring is filled by the engine's own steps (every commit gives its
    slots prio_max), the table is then set to random priorities, and one update is run.  Its `picked` and batch rows are the reference's on the
    table before the update and the Philox uniforms of (seed, update count 0), the weight column within the powf allowance; afterwards
    table[picked[b]] is the quantised delta of per_delta (the maximum where two batch episodes read the same slot), every other entry is as
    before, and prio_max has followed"""
    from kinovagrasping_amd.pipeline import GraphedTrainer
    sim, policy, replay, eng = _setup()
    tr = GraphedTrainer(sim, policy, replay, eng, batch_episodes=8, overlap=False, prioritized=True, per_alpha=0.6, per_beta=0.4, per_eps=1e-3)
    assert replay.ep_prio is not None and replay.priority_max() == pr.PRIO_ONE
    for _ in range(26):
        eng.step()
    torch.cuda.synchronize()
    cnt, cap = replay.count, replay.capacity
    assert 2 * 64 <= cnt <= cap
    table0 = replay.priorities().cpu().numpy()
    assert (table0 == pr.PRIO_ONE).all()                                        # committed at prio_max, the rest as enabled
    r = _rng("lock step")
    table = r.randint(pr.PRIO_ONE // 100, 50 * pr.PRIO_ONE, cap + 1).astype(np.uint32)
    replay.ep_prio.view(torch.int32).copy_(torch.from_numpy(table.view(np.int32)).to(replay.device))
    H, n, B = replay.horizon, replay.n_steps, 8
    W = H - n
    assert int(tr.native.it.item()) == 0
    tr._learn_eager()
    torch.cuda.synchronize()
    ring = _host_ring(replay, table)
    seed = tr.sample_seed & (2 ** 64 - 1)
    ue, us = philox_uniforms(np.arange(B), 0x5a4d, seed, 0), philox_uniforms(np.arange(B * W), 0x5a4e, seed, 0).reshape(B, W)
    ref = pr.sample_prioritized_ref(B, H, n, ring, ue, us, 0.4)
    picked = tr.picked.cpu().numpy()
    assert picked.tolist() == ref[6].tolist()
    for k in range(5):
        assert tr.batch[k].cpu().numpy().tobytes() == ref[k].tobytes(), k
    check_weights(tr.batch[5].cpu().numpy(), ref[5], "lock-step trainer")
    delta = tr.per_delta.cpu().numpy()
    assert np.isfinite(delta).all() and (delta >= 0).all()
    after = replay.priorities().cpu().numpy()
    want = {}
    for b in range(B):
        want[int(picked[b])] = max(want.get(int(picked[b]), 0.0), pr.quantise_ref(delta[b], 1e-3, 0.6))
    for s, x in want.items():
        check_entry(after[s], x, f"slot {s}")
    others = np.setdiff1d(np.arange(cap + 1), list(want))
    assert (after[others] == table[others]).all()
    assert replay.priority_max() == max([pr.PRIO_ONE] + [int(after[s]) for s in want])
    print(f"\nPRIO lock step: picked {picked.tolist()}, delta {delta.tolist()}, entries {[int(after[s]) for s in picked]}")
    sim.close()


def test_free_running_trainer_keeps_the_priority_table_consistent():
    """AsyncTrainer(prioritized=True) on the same set-up, three launches of 13 env-steps with captured graphs: every committed slot holds a
    priority in [1, 2^32 - 1], prio_max is at least every entry (an entry is a past prio_max or a value an update wrote), updates did write,
    nothing was dropped and no pacing wait timed out; beta is annealed between launches through set_per_beta"""
    from kinovagrasping_amd.pipeline import AsyncTrainer
    sim, policy, replay, eng = _setup()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        tr = AsyncTrainer(sim, policy, replay, eng, batch_episodes=8, prioritized=True, per_beta=0.4)
    tr.capture()
    assert replay.priority_max() == pr.PRIO_ONE and (replay.priorities() == pr.PRIO_ONE).all()       # the warm-up updates left no trace
    for k in range(3):
        tr.set_per_beta(0.4 + 0.3 * k)
        tr.run(13)
        tr.flush()
        torch.cuda.synchronize()
    c = tr.counts()
    cnt, head, cap = replay.count, replay.head, replay.capacity
    assert 2 * 64 <= cnt <= cap and c["episodes_dropped"] == 0 and c["pacing_timeouts"] == 0 and c["episodes_kept"] == cnt
    slots = (head - cnt + np.arange(cnt)) % cap
    table, top = replay.priorities().cpu().numpy(), replay.priority_max()
    assert (table[slots] >= 1).all() and (table[slots] <= pr.U32_MAX).all() and top >= int(table[slots].max()) and top >= pr.PRIO_ONE
    changed = int((table[slots] != pr.PRIO_ONE).sum())
    weight = tr.batch[5].cpu().numpy()
    print(f"\nPRIO free running: {c}, updates {tr.updates}, prio_max {top / pr.PRIO_ONE:.3f}, {changed} of {cnt} entries written, weights {weight.min():.3f} .. {weight.max():.3f}")
    assert tr.updates == 39 and changed > 0 and float(tr.per_beta.item()) == pytest.approx(1.0)
    assert ((weight >= 0) & (weight <= 1)).all() and np.isfinite(tr.per_delta.cpu().numpy()).all()
    picked = tr.picked.cpu().numpy()
    assert ((picked >= 0) & (picked < cap)).all()
    sim.close()
