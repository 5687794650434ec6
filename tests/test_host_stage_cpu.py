"""The host pipeline's pure arithmetic (sknnr_amd/csrc/host_stage.h: tile cuts, staging copies, the push description) in a
stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer: tests/cpp/host_stage_main.cpp is compiled
against the header with g++ and run as a child.  Nothing is loaded into Python.  What the program checks is listed at
its head."""

from __future__ import annotations

import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SOURCE = os.path.join(ROOT, "tests", "cpp", "host_stage_main.cpp")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-pthread"]


def test_host_stage_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this machine")
    exe = str(tmp_path / "host_stage")
    built = subprocess.run([gxx, *FLAGS, "-I", os.path.join(ROOT, "sknnr_amd", "csrc"), SOURCE, "-o", exe],
                           capture_output=True, text=True)
    if built.returncode != 0 and ("-lasan" in built.stderr or "-lubsan" in built.stderr or "libasan" in built.stderr
                                  or "libubsan" in built.stderr):
        pytest.skip("g++ has no sanitizer runtime to link: " + built.stderr.strip().splitlines()[-1])
    assert built.returncode == 0, built.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-3000:]
    assert run.stderr == "", run.stderr[-3000:]  # (a sanitizer report, or a failed check)
    assert run.stdout.strip() == "host stage ok"
