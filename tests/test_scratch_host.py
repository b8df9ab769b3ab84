"""The scope-bound owners of sqmc_amd/csrc/dev_scratch.h on the host: tests/scratch_host_check.cpp, a stand-alone program with counting
stand-ins for the HIP calls, built with the host compiler under the address and undefined-behaviour sanitizers and run as a child."""
import os
import shutil
import subprocess


HERE = os.path.dirname(os.path.abspath(__file__))
PROPERTIES = ["scope exit frees everything behind one synchronise", "an empty owner does not synchronise", "drop frees once",
              "keep hands a buffer over", "a failing k-th allocation leaves nothing behind, for every k", "the failure is remembered until clear",
              "fail_at fires exactly once", "peak bytes", "host arrays are released unless committed", "event marks are destroyed on every path"]


def test_scratch_owner_on_the_host(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "scratch_host_check")
    # the sanitizer runtimes are linked in statically: the program carries its own checks whatever else the loader brings
    static = ["-static-libsan"] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
                          + static + [os.path.join(HERE, "scratch_host_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in PROPERTIES:
        assert "ok " + name in r.stdout, (name, r.stdout)
    assert "all ok" in r.stdout

