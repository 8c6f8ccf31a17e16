"""plane_staging.h and matte_args.h on the host: the lists of the caller's planes that
yrt_render_aovs, yrt_render_mattes, yrt_render_passes and yrt_render_light_groups stage for host
memory, and the arguments yrt_render_mattes refuses.

tools/check_plane_staging.cpp is compiled with the host compiler into a stand-alone program and
run; no GPU and no libyrt.so are involved. The program walks every matte key mask, layer count
and mem, every AOV and pass mask and 1 to 8 light groups, and for each does the entry point's
round trip with memcpy standing in for the copies (its header comment lists what it asserts).
"""
from __future__ import annotations

import shutil
import subprocess

from helpers import ROOT


def test_check_plane_staging_builds_and_passes(tmp_path):
    cxx = next((c for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "check_plane_staging"
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", str(ROOT / "tools" / "check_plane_staging.cpp"),
                    "-o", str(exe)], check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1] == "ok"
