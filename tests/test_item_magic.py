"""item_magic.h on the host: the division pairs the persistent grids' item paths use instead of
the emulated integer division (wavefront.hip, YRT_ITEM_MAGIC), against Python's integers.

tests/item_magic_check.cpp is compiled with the host compiler into a stand-alone program; no
GPU and no libyrt.so are involved. Checked: quotient and remainder at the numerators within
+-2 of the multiples of d near 0, 2^16, 2^24 and the top of the admitted range (2^31 - 1), a
full sweep of 2^20 numerators at either end of that range, the `exact` flag -- set for every
nmax below 2^31 and clear from 2^31 on, where the pair is shown to be wrong at n = 2^31 -- and
the per-frame decisions of make_item_magic.
"""
from __future__ import annotations

import shutil
import subprocess

import pytest

from helpers import ROOT

CSRC = ROOT / "yocto_raytracing_amd" / "csrc"
TOP = 2 ** 31 - 1  # magic_nmax
# 2^25: the tiles across a frame of 2^31 pixels that is one tile high (2^28 x 8)
DIVISORS = (1, 2, 3, 5, 7, 8, 9, 64, 240, 241, 4096, 2 ** 25)
ANCHORS = (0, 2 ** 16, 2 ** 24, TOP)
SWEEP = 2 ** 20


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("item_magic") / "item_magic_check"
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", f"-I{CSRC}", str(ROOT / "tests" / "item_magic_check.cpp"),
                    "-o", str(exe)], check=True, capture_output=True, text=True)

    def run(*args):
        r = subprocess.run([str(exe), *map(str, args)], check=True, capture_output=True, text=True, timeout=60)
        return [[int(v) for v in line.split()] for line in r.stdout.splitlines()]

    return run


def numerators(d, nmax):
    out = set()
    for a in ANCHORS:
        for k in range(a // d - 2, a // d + 3):
            for delta in range(-2, 3):
                n = k * d + delta
                if 0 <= n <= nmax:
                    out.add(n)
    out.update((0, nmax))
    return sorted(out)


@pytest.mark.parametrize("d", DIVISORS)
def test_quotient_and_remainder_at_the_multiple_boundaries(prog, d):
    ns = numerators(d, TOP)
    assert len(ns) >= 12 and ns[-1] == TOP
    (mul, shift, exact), *qr = prog("eval", d, TOP, *ns)
    assert exact == 1 and mul < 2 ** 32 and shift < 32
    assert [tuple(v) for v in qr] == [divmod(n, d) for n in ns]
    # the pair is the round-up one: ceil(2^(31 + shift) / d)
    assert mul == -(-(2 ** (31 + shift)) // d)


@pytest.mark.parametrize("d", DIVISORS)
def test_full_sweeps_at_both_ends_of_the_range(prog, d):
    for lo, hi in ((0, SWEEP), (TOP - SWEEP, TOP)):
        (bad, first), = prog("sweep", d, TOP, lo, hi)
        assert bad == 0, (d, lo, hi, first)


@pytest.mark.parametrize("d", DIVISORS)
def test_exact_flag_is_clear_exactly_where_the_pair_is_wrong(prog, d):
    for nmax in (0, 1, 2 ** 16, 2 ** 24, TOP):
        (_, _, exact), = prog("eval", d, nmax)
        assert exact == 1, (d, nmax)
    for nmax in (TOP + 1, 2 ** 32 - 1, 2 ** 33):
        (_, _, exact), (q, _) = prog("eval", d, nmax, TOP + 1)
        assert exact == 0, (d, nmax)
        assert q != (TOP + 1) // d  # 2 n wraps at n = 2^31: not exact there, as the flag says


def test_bad_divisors_are_never_exact(prog):
    for d in (0, 2 ** 31 + 1, 2 ** 32 - 1):
        (_, _, exact), = prog("eval", d, 100)
        assert exact == 0, d
    (mul, shift, exact), (q, r) = prog("eval", 2 ** 31, TOP, TOP)
    assert (exact, q, r) == (1, 0, TOP)


def test_frame_decisions(prog):
    def frame(spp, samples, tiles_x, band, npix, max_samples, rows, w=1920, h=1080, x0=0, y0=0):
        (on, div_ok, pow2, log2), = prog("frame", spp, samples, tiles_x, band, npix, max_samples, rows, w, h, x0, y0)
        return on, div_ok, pow2, log2

    c4 = 240 * 135 * 64
    assert frame(64, 8, 240, 1, c4, c4 * 64, 1080) == (1, 1, 1, 6)
    assert frame(16, 4, 240, 8, c4, c4 * 16, 1080) == (1, 1, 1, 4)
    assert frame(4, 2, 240, 8, c4, c4 * 4, 1080) == (1, 1, 1, 2)
    assert frame(1, 1, 1, 5, 64 * 25, 64 * 25, 200) == (1, 1, 1, 0)
    assert frame(9, 3, 12, 16, 12 * 9 * 64, 12 * 9 * 64 * 9, 72)[:3] == (1, 1, 0)  # the per-lane form
    # a frame whose pixels are not counted in 32 bits, or whose chunk's samples pass 2^31: the general code
    assert frame(1, 1, 2 ** 25, 1, 2 ** 32, 2 ** 29, 16)[0] == 0
    assert frame(1, 1, 2 ** 25, 1, 2 ** 32 - 64, 2 ** 29, 8)[0] == 1
    assert frame(64, 8, 240, 1, c4, 2 ** 31, 1080)[0] == 0
    # a window origin the host would refuse leaves the per-item range checks in place
    assert frame(64, 8, 240, 1, c4, c4 * 64, 1080, x0=-1)[1] == 0
    assert frame(64, 8, 240, 1, c4, c4 * 64, 1080, w=0)[1] == 0
