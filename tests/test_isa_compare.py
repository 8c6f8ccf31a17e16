"""tools/isa_dump.py --compare: the verdict on a kernel from its disassembly in two builds.

Three hand-written pairs through split_symbols and classify, the two functions the command
is made of: equal listings; the same instructions reordered, one addition's operands swapped;
one instruction more. No compiler runs and no GPU is needed."""
import importlib.util
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def _tool():
    spec = importlib.util.spec_from_file_location("yrt_isa_dump", ROOT / "tools" / "isa_dump.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


T = _tool()

PARENT = """
Disassembly of section .text:
<k>:
	s_load_dwordx2 s[0:1], s[4:5], 0x0
	v_mul_f32_e32 v7, v1, v2
	v_sub_f32_e32 v8, v1, v2
	v_add_f32_e32 v4, v0, v3
	v_mul_f32_e32 v5, v4, v7
	s_waitcnt lgkmcnt(0)
	global_store_dwordx2 v6, v[4:5], s[0:1] offset:16
	s_endpgm
"""
# the first multiplication one slot later, the addition's operands swapped
REORDERED = """
Disassembly of section .text:
<k>:
	s_load_dwordx2 s[0:1], s[4:5], 0x0
	v_sub_f32_e32 v8, v1, v2
	v_mul_f32_e32 v7, v1, v2
	v_add_f32_e32 v4, v3, v0
	v_mul_f32_e32 v5, v4, v7
	s_waitcnt lgkmcnt(0)
	global_store_dwordx2 v6, v[4:5], s[0:1] offset:16
	s_endpgm
"""
ONE_MORE = """
Disassembly of section .text:
<k>:
	s_load_dwordx2 s[0:1], s[4:5], 0x0
	v_mul_f32_e32 v7, v1, v2
	v_sub_f32_e32 v8, v1, v2
	v_add_f32_e32 v4, v0, v3
	v_mov_b32_e32 v9, v4
	v_mul_f32_e32 v5, v4, v7
	s_waitcnt lgkmcnt(0)
	global_store_dwordx2 v6, v[4:5], s[0:1] offset:16
	s_endpgm
"""
RES = {"vgpr": 8, "sgpr": 10, "vgpr_spill": 0, "sgpr_spill": 0, "private": 0, "lds": 0, "block": 256}


def _k(text):
    syms = T.split_symbols(text)
    assert list(syms) == ["k"]
    return syms["k"]


def test_equal_is_identical():
    v = T.classify(_k(PARENT), _k(PARENT), RES, dict(RES))
    assert v == T.Verdict("identical", 0, {}, {})


def test_reordered_with_swapped_operands_is_same_mix():
    v = T.classify(_k(PARENT), _k(REORDERED), RES, dict(RES))
    assert v.verdict == "same-mix" and v.mnemonics == {} and v.resources == {}
    assert v.differing == 2  # the moved multiplication and the swapped addition


def test_one_instruction_more_is_changed():
    v = T.classify(_k(PARENT), _k(ONE_MORE), RES, dict(RES))
    assert v.verdict == "changed" and v.mnemonics == {"v_mov_b32_e32": 1} and v.differing == 1


def test_a_resource_delta_alone_is_changed():
    v = T.classify(_k(PARENT), _k(PARENT), RES, {**RES, "vgpr": 9})
    assert v.verdict == "changed" and v.resources == {"vgpr": (8, 9)} and v.mnemonics == {}
