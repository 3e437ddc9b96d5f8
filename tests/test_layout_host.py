"""The layouts of the context's workspace blocks (coloc_amd/csrc/clc_carve.h, clc_layout.h) on the host: tests/host/layout_driver.cpp
measures every view with a cursor without a base, places it on an allocation of exactly that size, writes every array over its full
extent and reads it back -- under ASan + UBSan, as a program of its own (nothing is loaded into Python).  A layout whose size and
pointers disagree, whose arrays overlap or overrun, or whose pointers are less aligned than their rule (16 B rows, 8 B doubles, 256 B
for the bundle adjustment) fails; so does a range that one transfer carries when it lies differently in the device and the pinned view."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_view_measures_places_and_holds_its_arrays(tmp_path):
    exe = tmp_path / "layout_driver"
    # the headers under test are host code: the only place where sanitizers can run
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "coloc_amd", "csrc"), os.path.join(ROOT, "tests", "host", "layout_driver.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("layout ok:"), out.stdout
