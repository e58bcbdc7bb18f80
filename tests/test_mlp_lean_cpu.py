"""The lean LDS-free MLP entry points (include/kinova_rollout.h: kr_mlp3_forward_lean / kr_mlp3_backward_lean): exported by the built
library with the declared argument counts, declared in the header, and their tile pairs kept apart from the one-wave kernels'."""
import ctypes
import re
from pathlib import Path

from kinovagrasping_amd import mlp
from kinovagrasping_amd import sim as ks

ROOT = Path(__file__).resolve().parents[1]
DECLARED_ARGS = {"kr_mlp3_forward_lean": 24, "kr_mlp3_backward_lean": 21}


def _declarations():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "kinova_rollout.h").read_text(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(kr_\w+)\s*\(([^;]*?)\)\s*;", header, flags=re.S)}


def test_header_declares_the_lean_entry_points():
    decl = _declarations()
    for name, nargs in DECLARED_ARGS.items():
        assert name in decl, f"{name} is not declared in include/kinova_rollout.h"
        args = [a.strip() for a in decl[name].split(",")]
        assert len(args) == nargs, (name, len(args))
        assert args[-1] == "void *stream" and "int64_t scratch_floats" in args and "float *scratch" in args


def test_library_exports_the_lean_entry_points_with_the_declared_argument_counts():
    lib = ks.load_library()
    for name, nargs in DECLARED_ARGS.items():
        assert name in ks.ROLLOUT_EXPORTS
        fn = getattr(lib, name)                    # AttributeError: not exported
        assert fn.restype == ctypes.c_int and len(fn.argtypes) == nargs, (name, len(fn.argtypes))
    # n <= 0 is a no-op before any pointer is looked at: callable without a GPU
    assert lib.kr_mlp3_forward_lean(0, 82, 0, 400, 300, 4, *([None] * 1), 82, None, 0, *([None] * 6), 0, 1.0, None, None, None, None, 0, None) == 0
    assert lib.kr_mlp3_backward_lean(0, 82, 400, 300, 4, *([None] * 8), 0, 0, None, 1.0, None, None, 0, None) == 0


def test_lean_tiles_are_disjoint_from_the_one_wave_tiles():
    assert mlp.LEAN_TILES == {(25, 19)}
    assert not (mlp.LEAN_TILES & mlp.SHADOW_TILES)
    assert mlp.LEAN_TILES <= mlp.SUPPORTED_TILES       # the LDS kernel and the in-kernel actor take the same widths
