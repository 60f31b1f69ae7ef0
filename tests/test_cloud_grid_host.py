"""The cell arithmetic of the point-cloud grid (numbotics_amd/csrc/nbk_cloud_grid.hpp) checked without a device:
tests/cloud_grid_check.cpp, a stand-alone program that includes that header alone, is built with AddressSanitizer and
UndefinedBehaviorSanitizer and run as a child process.  What it sweeps and holds is listed at its top; the library itself is not
loaded here."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "numbotics_amd", "csrc", "nbk_cloud_grid.hpp")


def test_cloud_grid_header_alone_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "cloud_grid_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cloud_grid_check.cpp"), "-o", exe], check=True, cwd=os.path.join(ROOT, "tests"))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[1] == "checks," and int(last[0]) > 100000 and last[2:] == ["0", "failed"], r.stdout[-400:]


def test_cloud_grid_header_has_no_device_code():
    """g++ alone compiles it (above); and it names no HIP type, call or kernel qualifier, and includes nothing of the project."""
    with open(HEADER, encoding="utf-8") as f:
        text = f.read()
    for word in ("hip_runtime", "hipStream", "hipLaunch", "hipError", "hipFunction", "hipMalloc", "__global__", "__device__", "__host__",
                 "g_opt", "getenv", '#include "'):
        assert word not in text, word
