"""The episode log without a GPU (include/kinova_sim.h: ks_set_episode_log / ks_get_episode_log, ks_episode_record): both libraries export
the entry points, the record's C layout is the ctypes mirror's, the ring decode (sim.decode_episode_ring) gives the unread records oldest
first with the exact number of lost ones, and metrics.EpisodeLedger folds records into the per-object and [N, K] tables and the
heatmap coordinate files."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from kinovagrasping_amd import build as kb
from kinovagrasping_amd import metrics
from kinovagrasping_amd import sim as ks

ROOT = Path(__file__).resolve().parents[1]
FIELDS = ("env", "object", "start_index", "steps", "done", "start_x", "start_y", "episode")


@pytest.mark.parametrize("multi_geom", [False, True])
def test_both_libraries_export_the_entry_points(multi_geom):
    kb.build()
    lib = ks.load_library(multi_geom=multi_geom)
    for name in ("ks_set_episode_log", "ks_get_episode_log"):
        assert hasattr(lib, name), name
        assert name in ks.EXPORTS


def test_record_layout_is_the_ctypes_mirror(tmp_path):
    """sizeof(ks_episode_record) == 32, every field a 32-bit word at the offset of the header's table - printed by a C program compiled
    against the header and compared with sim.KsEpisodeRecord; KS_EPISODE_LOG_CAPACITY_MAX, the limit the library checks, is sim.py's"""
    assert C.sizeof(ks.KsEpisodeRecord) == 32 and ks.EPISODE_RECORD_WORDS * 4 == 32
    assert [f[0] for f in ks.KsEpisodeRecord._fields_] == list(FIELDS)
    src = tmp_path / "record_layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kinova_sim.h"\n'
                   "typedef char record_is_32_bytes[sizeof(ks_episode_record) == 32 ? 1 : -1];\n"
                   "int main(void) {\n  ks_episode_record r;\n"
                   '  printf("%d", (int)sizeof(ks_episode_record));\n' +
                   "".join(f'  printf(" %d:%d", (int)offsetof(ks_episode_record, {f}), (int)sizeof r.{f});\n' for f in FIELDS) +
                   '  printf(" %d", (int)KS_EPISODE_LOG_CAPACITY_MAX);\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "record_layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60).stdout.split()
    assert out[0] == "32"
    assert int(out.pop()) == ks.EPISODE_LOG_CAPACITY_MAX == 1 << 24
    got = [tuple(int(x) for x in o.split(":")) for o in out[1:]]
    assert got == [(4 * i, 4) for i in range(8)]
    assert got == [(getattr(ks.KsEpisodeRecord, f).offset, getattr(ks.KsEpisodeRecord, f).size) for f in FIELDS]


def _ring(capacity, written):
    """what a ring of `capacity` slots holds after tickets 0 .. written - 1: word 0 = the ticket, word 7 = ticket * 3, floats in 5, 6"""
    ring = torch.zeros(capacity, 8, dtype=torch.int32)
    for t in range(written):
        row = torch.tensor([t, t % 5, t % 7 - 1, 5 + t % 3, 1 + t % 2, 0, 0, 3 * t], dtype=torch.int32)
        row[5:7] = torch.tensor([0.25 * t, -0.5 * t], dtype=torch.float32).view(torch.int32)
        ring[t % capacity] = row
    return ring


def test_ring_decode_without_a_wrap():
    words, lost = ks.decode_episode_ring(_ring(16, 10), 10, 0, 16)
    assert lost == 0 and words[:, 0].tolist() == list(range(10))
    words, lost = ks.decode_episode_ring(_ring(16, 10), 10, 4, 16)              # the reader had seen tickets 0..3
    assert lost == 0 and words[:, 0].tolist() == list(range(4, 10))
    rec = ks.episode_records(words)
    assert rec["env"].tolist() == list(range(4, 10)) and rec["episode"].tolist() == [3 * t for t in range(4, 10)]
    assert rec["object"].tolist() == [t % 5 for t in range(4, 10)] and rec["start_index"].tolist() == [t % 7 - 1 for t in range(4, 10)]
    assert rec["steps"].tolist() == [5 + t % 3 for t in range(4, 10)] and rec["done"].tolist() == [1 + t % 2 for t in range(4, 10)]
    assert rec["start_xy"].dtype == torch.float32 and rec["start_xy"].tolist() == [[0.25 * t, -0.5 * t] for t in range(4, 10)]


def test_ring_decode_across_the_wrap():
    # 21 tickets into 16 slots: slots 0..4 hold tickets 16..20; a reader at ticket 9 gets 9..20 in order, nothing lost
    words, lost = ks.decode_episode_ring(_ring(16, 21), 21, 9, 16)
    assert lost == 0 and words[:, 0].tolist() == list(range(9, 21))
    # exactly at the edge: cursor = written - capacity
    words, lost = ks.decode_episode_ring(_ring(16, 21), 21, 5, 16)
    assert lost == 0 and words[:, 0].tolist() == list(range(5, 21))


def test_ring_decode_with_a_cursor_older_than_the_ring():
    words, lost = ks.decode_episode_ring(_ring(16, 53), 53, 7, 16)
    assert lost == 53 - 7 - 16 and words[:, 0].tolist() == list(range(37, 53))
    words, lost = ks.decode_episode_ring(_ring(16, 53), 53, 0, 16)
    assert lost == 37 and words.shape == (16, 8)
    words, lost = ks.decode_episode_ring(_ring(16, 21), 21, 4, 16)              # one record lost
    assert lost == 1 and words[:, 0].tolist() == list(range(5, 21))


def test_ring_decode_of_an_empty_read():
    for written, cursor in ((0, 0), (10, 10), (53, 53)):
        words, lost = ks.decode_episode_ring(_ring(16, written), written, cursor, 16)
        assert lost == 0 and words.shape == (0, 8)
        rec = ks.episode_records(words)
        assert rec["env"].numel() == 0 and rec["start_xy"].shape == (0, 2)
    with pytest.raises(ValueError):
        ks.decode_episode_ring(_ring(16, 3), 3, 4, 16)                          # a cursor ahead of the log
    with pytest.raises(ValueError):
        ks.decode_episode_ring(torch.zeros(15, 8, dtype=torch.int32), 3, 0, 16)


def _records(rows):
    """rows of (env, object, start_index, steps, done, x, y)"""
    a = np.asarray(rows, dtype=np.float64)
    i32 = lambda c: torch.as_tensor(a[:, c].astype(np.int32))
    return {"env": i32(0), "object": i32(1), "start_index": i32(2), "steps": i32(3), "done": i32(4),
            "start_xy": torch.as_tensor(a[:, 5:7].astype(np.float32)), "episode": torch.zeros(len(rows), dtype=torch.int32)}


def test_ledger_tables_on_synthetic_records():
    # 4 envs, 3 objects (env e holds object e % 3), K = 2
    rows = [(0, 0, 0, 10, 1, 0.01, 0.02), (0, 0, 1, 30, 2, 0.03, 0.04), (1, 1, 1, 12, 1, 0.05, 0.06), (2, 2, 0, 30, 2, 0.07, 0.08),
            (3, 0, 1, 30, 3, 0.09, 0.10), (1, 1, 1, 30, 2, 0.11, 0.12), (0, 0, 0, 20, 1, 0.13, 0.14)]
    led = metrics.EpisodeLedger(4, 3, starts_per_env=2)
    led.add(_records(rows[:3]))
    r2 = _records(rows[3:])
    r2["lost"] = 2
    led.add(r2)
    assert led.episodes == 7 and led.successes == 4 and led.lost == 2 and led.success_rate() == 4 / 7      # done 3 = lifted at the time limit
    per = led.per_object(["a", "b", "c"])
    assert per == {"a": {"attempts": 4, "successes": 3, "mean_steps": 90 / 4}, "b": {"attempts": 2, "successes": 1, "mean_steps": 21.0},
                   "c": {"attempts": 1, "successes": 0, "mean_steps": 30.0}}
    assert led.attempts_table.tolist() == [[2, 1], [0, 2], [1, 0], [0, 1]]
    assert led.successes_table.tolist() == [[2, 0], [0, 1], [0, 0], [0, 1]]
    assert int(led.attempts_table.sum()) == led.episodes
    # an empty read changes nothing; a ledger that never saw a record reports zeros
    led.add(_records(np.zeros((0, 7))))
    assert led.episodes == 7
    assert metrics.EpisodeLedger(4, 2).per_object() == {0: {"attempts": 0, "successes": 0, "mean_steps": 0.0}, 1: {"attempts": 0, "successes": 0, "mean_steps": 0.0}}
    # records without a pool entry: totals and objects only
    led0 = metrics.EpisodeLedger(4, 3, starts_per_env=2)
    led0.add(_records([(2, 2, -1, 9, 1, 0.0, 0.0)]))
    assert led0.episodes == 1 and int(led0.attempts_table.sum()) == 0 and led0.per_object()[2]["successes"] == 1


def test_ledger_coords_go_through_save_heatmap_coords(tmp_path):
    rows = [(0, 0, 0, 10, 1, 0.01, 0.02), (0, 0, 1, 30, 2, 0.03, 0.04), (1, 0, 1, 12, 1, 0.05, 0.06), (2, 0, 0, 30, 2, 0.07, 0.08),
            (3, 0, 1, 30, 1, 0.09, 0.10), (1, 0, 0, 30, 2, 0.11, 0.12)]
    classes = np.array([["normal", "rotated", "top", "normal"], ["top", "normal", "normal", "rotated"]])       # [K, N] as scenarios.draw_start_pool returns
    led = metrics.EpisodeLedger(4, 1, starts_per_env=2).add(_records(rows))
    ok, fail = led.coords(classes)
    f32 = lambda v: [float(np.float32(x)) for x in v]
    assert ok == {"x": f32([0.01, 0.05, 0.09]), "y": f32([0.02, 0.06, 0.10]), "orientation": ["normal", "normal", "rotated"]}
    assert fail == {"x": f32([0.03, 0.07, 0.11]), "y": f32([0.04, 0.08, 0.12]), "orientation": ["top", "top", "rotated"]}
    text = metrics.save_heatmap_coords(ok, fail, 60, tmp_path)
    assert "Total # Success: 3" in text and "Total # Fail: 3" in text
    assert "Normal Orientation\n# Success: 2\n# Fail: 0" in text and "Rotated Orientation\n# Success: 1\n# Fail: 1" in text
    assert "Top Orientation\n# Success: 0\n# Fail: 2" in text
    assert (tmp_path / "heatmap_info.txt").read_text() == text
    assert np.load(tmp_path / "normal" / "success_x_60.npy").tolist() == f32([0.01, 0.05])
    assert np.load(tmp_path / "rotated" / "fail_y_60.npy").tolist() == f32([0.12])
    assert np.load(tmp_path / "top" / "fail_x_60.npy").tolist() == f32([0.03, 0.07])
    assert not (tmp_path / "top" / "success_x_60.npy").exists()
    # one class for everything / one per env; clear empties the coordinates and keeps the tables
    ok1, fail1 = led.coords("normal")
    assert set(ok1["orientation"]) == {"normal"} and len(fail1["x"]) == 3
    ok2, _ = led.coords(["top", "rotated", "normal", "normal"], clear=True)
    assert ok2["orientation"] == ["top", "rotated", "normal"]
    assert led.coords(classes) == ({"x": [], "y": [], "orientation": []}, {"x": [], "y": [], "orientation": []}) and led.episodes == 6
    with pytest.raises(ValueError):
        metrics.EpisodeLedger(4, 1).add(_records([(0, 0, -1, 5, 2, 0, 0)])).coords(classes)
