"""The LDS layouts of the kernels (numbotics_amd/csrc/nbk_lds.hpp: one struct per kernel family, read by the kernel's carve, the
launch's byte count, the entry point's refusal and creation's verdicts) checked without a device: tests/lds_check.cpp, a stand-alone
program that includes that header alone, is built with AddressSanitizer and UndefinedBehaviorSanitizer and run as a child process.
What it sweeps and holds is listed at its top; the library itself is not loaded here."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "numbotics_amd", "csrc", "nbk_lds.hpp")


def test_lds_header_alone_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "lds_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "lds_check.cpp"), "-o", exe], check=True, cwd=os.path.join(ROOT, "tests"))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    last = lines[-1].split()
    assert last[1] == "checks," and int(last[0]) >= 100000 and last[2:] == ["0", "failed"], r.stdout[-400:]
    # "creation implies fit" has one exemption, which the program asserts to be exactly this case and reports on one line: the sweep meets it
    exempt = [ln for ln in lines if ln.startswith("exempt:")]
    assert len(exempt) == 1, r.stdout[-400:]
    m = re.fullmatch(r"exempt: k_edges launched beyond LDS_MAX for a robot without pairs and without the parked layout: (\d+) descriptors", exempt[0])
    assert m is not None and int(m.group(1)) > 0, exempt[0]


def test_lds_header_has_no_device_code():
    """g++ alone compiles it (above); it includes nothing of the project and names no HIP type or call.  The kernels read it too, so its
    functions carry one qualifier macro: the two lines that define NBK_HD are the only place a kernel qualifier may stand."""
    with open(HEADER, encoding="utf-8") as f:
        text = f.read()
    define = "#ifdef __HIPCC__\n#define NBK_HD __host__ __device__\n#else\n#define NBK_HD\n#endif\n"
    assert text.count(define) == 1
    rest = text.replace(define, "")
    for word in ("hip_runtime", "hipStream", "hipLaunch", "hipError", "hipFunction", "hipMalloc", "__global__", "__device__", "__host__", "__shared__",
                 "__HIPCC__", "g_opt", "getenv", '#include "'):
        assert word not in rest, word
    assert re.findall(r"#include\s*<([^>]+)>", rest) == ["stddef.h"]
