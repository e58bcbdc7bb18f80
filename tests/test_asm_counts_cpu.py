"""tools/asm_counts.py on a hand-made piece of assembly (no compiler run): what counts as an instruction, how encodings are folded, that a DPP
multiply-add is the v_fma_f32 it replaces, where registers and scratch are read, and that the diff judges the arithmetic alone."""
import importlib.util
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
spec = importlib.util.spec_from_file_location("asm_counts", ROOT / "tools" / "asm_counts.py")
ac = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ac)

OLD = """\t.text
\t.p2align\t2                               ; -- Begin function _Z1kv
\t.type\t_Z1kv,@function
_Z1kv:                                  ; @_Z1kv
; %bb.0:
\tv_mov_b32_e32 v1, 0
\ts_nop 1
\tv_mov_b32_dpp v1, v0 row_newbcast:3 row_mask:0xf bank_mask:0xf
\tv_fma_f32 v2, -v1, v3, v2
\tv_pk_mul_f32 v[4:5], v[4:5], v[6:7]
\tv_sub_f32_e32 v8, v8, v4
\tv_add_f32_dpp v9, v9, v9 row_ror:8 row_mask:0xf bank_mask:0xf
.LBB0_1:
\t;;#ASMSTART
\t;;#ASMEND
\tv_add_u32_e32 v10, 1, v10
\ts_endpgm
.Lfunc_end0:
\t.size\t_Z1kv, .Lfunc_end0-_Z1kv
; NumVgprs: 11
; NumAgprs: 2
; ScratchSize: 16
\tv_mul_f32_e32 v0, v0, v0
"""
# the same arithmetic: the zero-initialising move gone, the broadcast folded into a DPP multiply-add
NEW = OLD.replace("\tv_mov_b32_e32 v1, 0\n", "").replace(
    "\tv_mov_b32_dpp v1, v0 row_newbcast:3 row_mask:0xf bank_mask:0xf\n\tv_fma_f32 v2, -v1, v3, v2\n",
    "\tv_fmac_f32_dpp v2, v0, -v3 row_newbcast:3 row_mask:0xf bank_mask:0xf\n")


def counts(tmp_path, text, name="a.s"):
    p = tmp_path / name
    p.write_text(text)
    return ac.count(p)


def test_counts_of_one_function(tmp_path):
    c = counts(tmp_path, OLD)["_Z1kv"]
    assert c["n"] == 9                                  # no directive, label, comment or asm marker; nothing behind .Lfunc_end
    assert (c["mov"], c["dpp_mov"], c["nop"]) == (1, 1, 1)
    assert dict(c["fp"]) == {"v_fma_f32": 1, "v_pk_mul_f32": 1, "v_sub_f32": 1, "v_add_f32": 1}
    assert (c["vgpr"], c["agpr"], c["scratch"]) == (11, 2, 16)


def test_a_dpp_multiply_add_is_the_fma_it_replaces(tmp_path, capsys):
    old, new = counts(tmp_path, OLD, "old.s"), counts(tmp_path, NEW, "new.s")
    assert new["_Z1kv"]["n"] == 7 and new["_Z1kv"]["fp"] == old["_Z1kv"]["fp"]
    assert ac.fold("v_fmac_f32_e32") == "v_fmac_f32" and ac.fold("v_mul_f32_dpp") == "v_mul_f32"
    names = {"_Z1kv": "k"}
    assert ac.diff(new, old, names, None) == 0
    assert "equal (4 ops)" in capsys.readouterr().out


def test_the_diff_fails_on_a_moved_rounding_only(tmp_path, capsys):
    unfused = OLD.replace("\tv_fma_f32 v2, -v1, v3, v2\n", "\tv_mul_f32_e32 v11, v1, v3\n\tv_sub_f32_e32 v2, v2, v11\n")
    old, new = counts(tmp_path, OLD, "old.s"), counts(tmp_path, unfused, "new.s")
    assert ac.diff(new, old, {"_Z1kv": "k"}, None) == 1
    out = capsys.readouterr().out
    assert "v_fma_f32 1 -> 0" in out and "v_sub_f32 1 -> 2" in out and "v_mul_f32 0 -> 1" in out
    more_moves = OLD.replace("\ts_nop 1\n", "\ts_nop 1\n\tv_mov_b32_e32 v12, v1\n\ts_nop 0\n")
    assert ac.diff(counts(tmp_path, more_moves, "m.s"), old, {"_Z1kv": "k"}, None) == 0
