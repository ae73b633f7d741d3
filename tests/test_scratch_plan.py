"""The censuses' scratch carver and rows-per-wave plan (kaboodle_amd/csrc/kb_scratch.h: no HIP in it) as a stand-alone
program, built with AddressSanitizer and UBSan; and the library build knows the frame's headers."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_carver_and_planner_under_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "scratch_plan")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cpp", "scratch_plan_main.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "scratch plan ok" in out.stdout, out.stdout + out.stderr


def test_the_build_lists_every_header_the_unit_includes():
    from kaboodle_amd import build
    listed = {os.path.basename(p) for p in build.deps()}
    csrc = os.path.join(ROOT, "kaboodle_amd", "csrc")
    assert {f for f in os.listdir(csrc) if f.endswith(".h")} <= listed
