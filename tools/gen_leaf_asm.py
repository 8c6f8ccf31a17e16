"""Generate yocto_raytracing_amd/csrc/leaf_asm.h: the triangle loops of the two nested walks'
shape leaves (packet_trace.h packet_first_list and packet_occluded_nested, YRT_LEAF_ASM) as one
inline-assembly "leaf scan" block each, so that the scalar unit issues only what a triangle
needs.

    python tools/gen_leaf_asm.py        (rewrites the header; build.py does not run it)

Why assembly: compiled, a triangle that no lane passes at the first barycentric test costs 19
scalar-side instructions (loads, waits and branches included): every compare is balloted into
an SGPR pair, the pairs are ANDed with the leaf's lane mask and the result is compared against 0
again, and the loop's index, record offset and end are kept apart. Here EXEC is the leaf's lane
mask for the whole scan, the compares are `v_cmpx` (EXEC narrows to the lanes that pass, and
the exits branch on EXEC being empty), and the loop runs on the record's byte offset alone: 10
scalar-side instructions per triangle at the first exit.

Both blocks scan the triangles at byte offsets off .. end of the leaf and do, per triangle,
exactly tri_hit_mask<true>'s / tri_hit_nb<true>'s operations in their order: cross and dot as
separate multiplies, subtractions and additions (no fma: the reference's build has none), the
reciprocal as fast_div.h's rcp_nr (v_rcp_f32 and its two fma), c = o - v0, and the three stages
with their wave-wide exits. `den != 0` is not tested: the scan leaves for the compiled code
whenever some lane of the mask fails rcp_nr_ok, and a lane that passes it has a normal,
non-zero den. The compiled tri_hit_mask / tri_hit_nb then handles that one triangle, IEEE
division included, and the scan is entered again behind it.

  closest hit   records of 3 x f4 (v0|ei, e1, e2) from S.sprims. When some lane hits triangle
                `off`, hm (the lanes), t, w1 and w2 come back; the compiled code reads the
                element word, does the five selects and enters the scan again at off + 48.
  any hit       records of 9 packed dwords (v0, e1, e2) from S.aprims. The lanes that hit are
                ORed into `gone` and leave the leaf's mask; the scan ends early when the mask is
                empty (a lane's answer does not change: it is already occluded).
No status word comes back (an SGPR the kernels do not have): hm != 0 is a hit, off < end
without one the compiled code's triangle, off >= end the end of the leaf (the any hit sets
off = end when it ends because every lane is answered).

Registers: the record in s16-s27 (s16-s24 for the any hit), the caller's EXEC in s[28:29] --
the range the descent blocks clobber, dead between descents. EXEC is restored before the
block ends. Hazard spacing: the record's SGPRs are read by the VALU after `s_waitcnt` and one
`s_nop`, as the compiler spaces its own scalar loads; three independent subtractions stand
between v_rcp_f32 and the fma that reads it. The stages behind the first exit lie behind the
loop's back branch, so the common path falls through.
"""
from __future__ import annotations

from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
OUT = ROOT / "yocto_raytracing_amd" / "csrc" / "leaf_asm.h"

D = ("%[dx]", "%[dy]", "%[dz]")
O = ("%[ox]", "%[oy]", "%[oz]")
R = ("%[r0]", "%[r1]", "%[r2]")  # r = cross(d, e2), then s = cross(c, e1)
C = ("%[c0]", "%[c1]", "%[c2]")
TMP = "%[t]"  # a product on its way into a sum, until stage 3 makes it t

# the records' SGPRs: closest hit {v0.xyz, ei} {e1.xyz, -} {e2.xyz, -}; any hit v0 e1 e2 packed
REC = {
    "first": {"v0": ("s16", "s17", "s18"), "ei": "s19", "e1": ("s20", "s21", "s22"), "e2": ("s24", "s25", "s26"),
              "loads": ["s_load_dwordx8 s[16:23], %[pb], %[off]", "s_load_dwordx4 s[24:27], %[pb], %[off] offset:0x20"],
              "stride": 48},
    "any": {"v0": ("s16", "s17", "s18"), "e1": ("s19", "s20", "s21"), "e2": ("s22", "s23", "s24"),
            "loads": ["s_load_dwordx8 s[16:23], %[pb], %[off]", "s_load_dword s24, %[pb], %[off] offset:0x20"],
            "stride": 36},
}
SAVED_EXEC = "s[28:29]"


def cross(dst, a, b, tmp=TMP) -> list[str]:
    """dst = {a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x}; b may be SGPRs"""
    L = []
    for k in range(3):
        i, j = (k + 1) % 3, (k + 2) % 3
        L.append(f"v_mul_f32 {dst[k]}, {b[j]}, {a[i]}")
        L.append(f"v_mul_f32 {tmp}, {b[i]}, {a[j]}")
        L.append(f"v_sub_f32 {dst[k]}, {dst[k]}, {tmp}")
    return L


def dot(dst, a, b, tmp=TMP) -> list[str]:
    """dst = (a.x b.x + a.y b.y) + a.z b.z; b may be SGPRs"""
    return [f"v_mul_f32 {dst}, {b[0]}, {a[0]}", f"v_mul_f32 {tmp}, {b[1]}, {a[1]}", f"v_add_f32 {dst}, {dst}, {tmp}",
            f"v_mul_f32 {tmp}, {b[2]}, {a[2]}", f"v_add_f32 {dst}, {dst}, {tmp}"]


def stage1(walk: str) -> list[str]:
    """den, the rcp_nr_ok check, 1/den, c, w1 and its range: EXEC = the lanes that pass"""
    r = REC[walk]
    L = cross(R, D, r["e2"])
    L += dot("%[w2]", R, r["e1"])  # den, in w2's register until stage 2
    # rcp_nr_ok: (|den| bits) - 0x00800000 < 0x7e000000, unsigned; a lane of the mask outside it
    # (a zero, a denormal, a huge value, a NaN): the compiled code's triangle
    L.append(f"v_and_b32 {TMP}, 0x7fffffff, %[w2]")
    L.append(f"v_add_u32 {TMP}, 0xff800000, {TMP}")
    L.append(f"v_cmp_le_u32 vcc, 0x7e000000, {TMP}")
    L.append("s_cbranch_vccnz .Lyl_slow%=")
    L.append("v_rcp_f32 %[inv], %[w2]")
    for k in range(3):
        L.append(f"v_subrev_f32 {C[k]}, {r['v0'][k]}, {O[k]}")  # c = o - v0
    L.append(f"v_fma_f32 {TMP}, -%[w2], %[inv], 1.0")  # rcp_nr's two fma
    L.append(f"v_fma_f32 %[inv], {TMP}, %[inv], %[inv]")
    L += dot("%[w1]", R, C)
    L.append("v_mul_f32 %[w1], %[w1], %[inv]")
    L.append("v_cmpx_ngt_f32 vcc, 0, %[w1]")  # !(w1 < 0): a NaN passes, as in the reference
    L.append("v_cmpx_nlt_f32 vcc, 1.0, %[w1]")  # !(w1 > 1)
    return L


def stage2(walk: str) -> list[str]:
    r = REC[walk]
    L = cross(R, C, r["e1"])  # s
    L += dot("%[w2]", R, D)
    L.append("v_mul_f32 %[w2], %[w2], %[inv]")
    L.append("v_cmpx_ngt_f32 vcc, 0, %[w2]")  # !(w2 < 0)
    L.append(f"v_add_f32 {TMP}, %[w1], %[w2]")
    L.append(f"v_cmpx_nlt_f32 vcc, 1.0, {TMP}")  # !(w1 + w2 > 1)
    return L


def stage3(walk: str) -> list[str]:
    r = REC[walk]
    L = dot(TMP, R, r["e2"], tmp=C[0])
    L.append(f"v_mul_f32 {TMP}, {TMP}, %[inv]")
    L.append(f"v_cmpx_nlt_f32 vcc, {TMP}, %[tmin]")  # !(t < tmin)
    L.append(f"v_cmpx_ngt_f32 vcc, {TMP}, %[tmax]")  # !(t > tmax)
    return L


def body(walk: str) -> list[str]:
    r = REC[walk]
    L = [f"s_mov_b64 {SAVED_EXEC}, exec", "s_mov_b64 exec, %[lm]"]
    L.append(".Lyl_loop%=:")
    L += r["loads"]
    L.append("s_waitcnt lgkmcnt(0)")
    L.append("s_nop 0")
    L += stage1(walk)
    L.append("s_cbranch_execnz .Lyl_two%=")
    L.append(".Lyl_next%=:")
    L.append("s_mov_b64 exec, %[lm]")
    L.append(f"s_add_u32 %[off], %[off], {r['stride']}")
    L.append("s_cmp_lt_u32 %[off], %[end]")
    L.append("s_cbranch_scc1 .Lyl_loop%=")
    L.append(".Lyl_done%=:")  # off >= end says so (the any hit may end with triangles left: off = end)
    L.append("s_mov_b64 %[hm], 0" if walk == "first" else "s_mov_b32 %[off], %[end]")
    L.append("s_branch .Lyl_end%=")
    L.append(".Lyl_two%=:")
    L += stage2(walk)
    L.append("s_cbranch_execz .Lyl_next%=")
    L += stage3(walk)
    L.append("s_cbranch_execz .Lyl_next%=")
    if walk == "first":
        L.append("s_mov_b64 %[hm], exec")
        L.append("s_branch .Lyl_end%=")
        L.append(".Lyl_slow%=:")
        L.append("s_mov_b64 %[hm], 0")
    else:
        L.append("s_or_b64 %[gone], %[gone], exec")
        L.append("s_andn2_b64 %[lm], %[lm], exec")  # SCC = some lane of the leaf is still unanswered
        L.append("s_cbranch_scc1 .Lyl_next%=")
        L.append("s_branch .Lyl_done%=")
        L.append(".Lyl_slow%=:")
    L.append(".Lyl_end%=:")
    L.append(f"s_mov_b64 exec, {SAVED_EXEC}")
    return L


def first_exit_path(walk: str) -> list[str]:
    """one triangle that no lane passes at the first barycentric test: the loop label to the
    branch back"""
    b = body(walk)
    return b[b.index(".Lyl_loop%=:"): b.index("s_cbranch_scc1 .Lyl_loop%=") + 1]


CLOBBERS = ", ".join(f'"s{i}"' for i in range(16, 30)) + ',\n          "vcc", "scc", "exec"'
TEMPS_OUT = ('[r0] "=&v"(r0), [r1] "=&v"(r1), [r2] "=&v"(r2), [c0] "=&v"(c0), [c1] "=&v"(c1), [c2] "=&v"(c2),\n'
             '          [inv] "=&v"(inv)')
RAY_IN = ('[ox] "v"(o.x), [oy] "v"(o.y), [oz] "v"(o.z), [dx] "v"(d.x), [dy] "v"(d.y), [dz] "v"(d.z),\n'
          '          [tmin] "v"(tmin), [tmax] "v"(tmax)')


def emit(walk: str) -> str:
    lines = "\n".join(f'        "{x}\\n"' for x in body(walk))
    if walk == "first":
        return f"""// comes back with hm != 0: the lanes that hit triangle `off`, and their t, w1, w2 (the scan goes on
// at off + 48); with hm == 0 and off < end: triangle `off` is the compiled code's; else the leaf is done
__device__ __forceinline__ void leaf_scan_first(const f4* pb, uint32_t& off, uint32_t end, unsigned long long lm,
                                                vec3f o, vec3f d, float tmin, float tmax, unsigned long long& hm,
                                                float& t, float& w1, float& w2) {{
    float r0, r1, r2, c0, c1, c2, inv;
    off = (uint32_t)__builtin_amdgcn_readfirstlane((int)off);
    asm volatile(
{lines}
        : [off] "+s"(off), [hm] "=&s"(hm), [t] "=&v"(t), [w1] "=&v"(w1), [w2] "=&v"(w2),
          {TEMPS_OUT}
        : [pb] "s"(pb), [end] "s"(end), [lm] "s"(lm),
          {RAY_IN}
        : {CLOBBERS});
    // (SGPR outputs, said again: the compiler's uniformity analysis does not follow them)
    off = (uint32_t)__builtin_amdgcn_readfirstlane((int)off), hm = uniform64(hm);
}}
"""
    return f"""// lm: the leaf's lanes not yet answered; gone: the walk's answered lanes (the hits go in). Comes back
// with off < end: triangle `off` is the compiled code's; else the leaf, or every lane of it, is done
__device__ __forceinline__ void leaf_scan_any(const f4* pb, uint32_t& off, uint32_t end, unsigned long long& lm,
                                              unsigned long long& gone, vec3f o, vec3f d, float tmin, float tmax) {{
    float t, w1, w2, r0, r1, r2, c0, c1, c2, inv;
    off = (uint32_t)__builtin_amdgcn_readfirstlane((int)off), lm = uniform64(lm), gone = uniform64(gone);
    asm volatile(
{lines}
        : [off] "+s"(off), [lm] "+s"(lm), [gone] "+s"(gone), [t] "=&v"(t), [w1] "=&v"(w1), [w2] "=&v"(w2),
          {TEMPS_OUT}
        : [pb] "s"(pb), [end] "s"(end),
          {RAY_IN}
        : {CLOBBERS});
    // (SGPR outputs, said again: the compiler's uniformity analysis does not follow them)
    off = (uint32_t)__builtin_amdgcn_readfirstlane((int)off), lm = uniform64(lm), gone = uniform64(gone);
}}
"""


def main():
    parts = [
        "// leaf_asm.h -- GENERATED by tools/gen_leaf_asm.py (do not edit): the triangle loops of the\n"
        "// nested walks' shape leaves in one asm block each (packet_first_list, packet_occluded_nested,\n"
        "// YRT_LEAF_ASM; the generator's docstring says what they compute and why).\n"
        "#pragma once\n\n"
        "#include \"trace_common.h\"\n\n"
        "namespace yrt {\n\n"
        "__device__ __forceinline__ unsigned long long uniform64(unsigned long long v) {\n"
        "    return (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32 |\n"
        "           (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);\n"
        "}\n\n",
        emit("first"), "\n", emit("any"), "\n",
        "}  // namespace yrt\n",
    ]
    OUT.write_text("".join(parts))
    print(OUT)


if __name__ == "__main__":
    main()
