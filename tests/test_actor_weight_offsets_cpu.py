"""The actor forward reads its weights, biases and input rows through range-checked buffer loads whose guards are all in the lane offset
(csrc/ks_mlp_tile.h: quad_off, tail_off, tail_here, x_off).  A lane offset that is wrong by one row or one word reads a neighbour's
weights - or faults - on the GPU, so the rule is walked on the host first: tests/native/ks_mlp_offsets.cpp plays every load of both tile
bodies (every lane, every tile including the prefetches behind the last one, every k-step; W1 at in_dim 82 / 86 / 96 / 5, W2 and W3 at nine
width pairs with partial last tiles and rows that are no whole quads, out_dim 1 - 4, the wave form's 4 rows and the 16-row form with 1 and
4 waves, batch rows < 0) against matrices with NaN on both sides, as its own executable under AddressSanitizer and UBSan."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def test_every_operand_load_of_the_actor_forward_stays_inside_its_matrix(tmp_path):
    exe = tmp_path / "ks_mlp_offsets"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe),
                           str(ROOT / "tests" / "native" / "ks_mlp_offsets.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
    loads, oor, failed = (int(w) for w in out.stdout.split() if w.isdigit())
    assert failed == 0 and loads > 1_000_000 and 0 < oor < loads
