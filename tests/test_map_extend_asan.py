"""coloc_amd/csrc/extend_math.h and grow_point (map_math.h) under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone
program (tests/host/map_extend_asan_main.cpp, its own main): host code only, nothing loaded into Python, no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_extend_math_is_clean_under_the_sanitizers(tmp_path):
    exe = tmp_path / "map_extend_asan_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "host", "map_extend_asan_main.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "map_extend_asan_main: ok" in r.stdout
