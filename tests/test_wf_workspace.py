"""wf_workspace.h on the host: the layout of the wavefront path's workspace, which run() and
run_rays() (wavefront.hip) size with one walk over its slabs and carve with the same walk.

tools/check_wf_workspace.cpp is compiled with the host compiler into a stand-alone program and
run; no GPU and no libyrt.so are involved. The program sweeps samples per pixel, lights, mirror
levels, pass planes, group planes and chunk sizes up to 2^29 samples, checks alignment, order
and the total of every shape, writes every slab of the small shapes, and compares the totals of
a fixed table of shapes with what the code before the header computed (its header comment lists
what it asserts).
"""
from __future__ import annotations

import shutil
import subprocess

from helpers import ROOT


def test_check_wf_workspace_builds_and_passes(tmp_path):
    cxx = next((c for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "check_wf_workspace"
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    f"-I{ROOT / 'yocto_raytracing_amd' / 'csrc'}", f"-I{ROOT / 'include'}",
                    str(ROOT / "tools" / "check_wf_workspace.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1] == "ok"
