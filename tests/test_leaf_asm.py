"""leaf_asm.h is generated: the committed header must be what tools/gen_leaf_asm.py writes (the
walks' parity tests run the committed header), and its two blocks must keep the shape the
generator's docstring describes. The counts are read from the generator's own instruction list."""
import importlib.util
import re

import pytest

from helpers import ROOT

HDR = ROOT / "yocto_raytracing_amd" / "csrc" / "leaf_asm.h"
WALKS = ("first", "any")
# scalar-side lines (SALU, SMEM, waits, nops, branches) of one triangle that no lane passes at the
# first barycentric test: two loads, the wait, the nop, the slow-path and first-exit branches, the
# EXEC reset, the offset's add and compare and the branch back. The compiled loops have 19
FIRST_EXIT_SCALAR = 10


def _gen():
    spec = importlib.util.spec_from_file_location("gen_leaf_asm", ROOT / "tools" / "gen_leaf_asm.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_header_is_generated(tmp_path, monkeypatch):
    gen = _gen()
    out = tmp_path / "leaf_asm.h"
    monkeypatch.setattr(gen, "OUT", out)
    gen.main()
    assert out.read_text() == HDR.read_text(), "leaf_asm.h differs from tools/gen_leaf_asm.py's output"


def test_one_block_per_walk():
    text = HDR.read_text()
    assert re.findall(r"void (leaf_scan_\w+)\(", text) == ["leaf_scan_first", "leaf_scan_any"]
    assert text.count("asm volatile(") == 2
    assert text.count(".Lyl_loop%=:") == 2


@pytest.mark.parametrize("walk", WALKS)
def test_scalar_work_per_triangle_at_the_first_exit(walk):
    gen = _gen()
    body = gen.body(walk)
    start, back = body.index(".Lyl_loop%=:"), body.index("s_cbranch_scc1 .Lyl_loop%=")
    path = body[start: back + 1]
    assert path == gen.first_exit_path(walk)
    scalar = [x for x in path if x.startswith("s_")]
    print(walk, len(scalar), scalar)
    assert len(scalar) <= 13  # the bound this change was taken on
    assert len(scalar) == FIRST_EXIT_SCALAR, scalar
    # the exits read EXEC after v_cmpx (and VCC for the reciprocal's range): no mask is ANDed or
    # compared against 0 on this path, and nothing else branches away from it
    assert not any(x.startswith(("s_and", "s_cmp_lg_u64", "s_cmp_eq_u64")) for x in path)
    branches = [x for x in path if x.startswith(("s_cbranch", "s_branch"))]
    assert branches == ["s_cbranch_vccnz .Lyl_slow%=", "s_cbranch_execnz .Lyl_two%=", "s_cbranch_scc1 .Lyl_loop%="]


@pytest.mark.parametrize("walk", WALKS)
def test_no_fused_multiply_add_but_the_reciprocal_s(walk):
    body = _gen().body(walk)
    fused = [x for x in body if re.match(r"v_(fma|fmac|mac|mad)", x)]
    assert len(fused) == 2 and all(x.startswith("v_fma_f32") for x in fused), fused
    # both directly behind v_rcp_f32's three independent subtractions (c = o - v0)
    k = body.index(fused[0])
    assert body[k + 1] == fused[1]
    assert body[k - 4].startswith("v_rcp_f32") and all(x.startswith("v_subrev_f32") for x in body[k - 3: k])
    # cross, dot: 6 + 3 products per cross / dot pair, each its own instruction
    assert sum(x.startswith("v_mul_f32") for x in body) == 2 * 6 + 4 * 3 + 3  # + the three `* inv_den`
    assert sum(x.startswith(("v_sub_f32", "v_add_f32")) for x in body) == 2 * 3 + 4 * 2 + 1  # + w1 + w2


def test_any_hit_keeps_its_hits_as_a_scalar_mask():
    body = _gen().body("any")
    assert not any("v_cndmask" in x or x.startswith("v_or") for x in body)
    assert "s_or_b64 %[gone], %[gone], exec" in body
    # the lanes that hit leave the leaf's mask, and the scan ends when it is empty
    k = body.index("s_andn2_b64 %[lm], %[lm], exec")
    assert body[k + 1] == "s_cbranch_scc1 .Lyl_next%="


@pytest.mark.parametrize("walk", WALKS)
def test_exec_is_saved_first_and_restored_last(walk):
    gen = _gen()
    body = gen.body(walk)
    assert body[0] == f"s_mov_b64 {gen.SAVED_EXEC}, exec"
    assert body[-1] == f"s_mov_b64 exec, {gen.SAVED_EXEC}" and body[-2] == ".Lyl_end%=:"
    # every way out goes through the end label: no other label follows a branch out of the block
    targets = {x.split()[-1] for x in body if x.startswith(("s_branch", "s_cbranch"))}
    labels = {x[:-1] for x in body if x.endswith(":")}
    assert targets <= labels
    # only the scratch range the descent blocks clobber is named (s16-s29), and it is declared
    named = {int(n) for x in body for n in re.findall(r"\bs(\d+)\b", x)}
    named |= {n for x in body for a, b in re.findall(r"s\[(\d+):(\d+)\]", x) for n in range(int(a), int(b) + 1)}
    assert named and named <= set(range(16, 30)), sorted(named)
    assert all(f'"s{n}"' in gen.CLOBBERS for n in named) and '"exec"' in gen.CLOBBERS
