"""The host arithmetic of sqmc_gpu_hci_2rdm (sqmc_amd/csrc/rdm2_plan.h: records and pairs per block, the width of the intermediate
key, one sort word or two passes, the order of the columns): tests/rdm2_host_check.cpp, a stand-alone program built with the host
compiler under the address and undefined-behaviour sanitizers and run as a child."""
import os
import shutil
import subprocess


HERE = os.path.dirname(os.path.abspath(__file__))
PROPERTIES = ["binomials up to 64", "key widths", "shapes of every sector", "one word, two passes, refused", "column order"]


def test_rdm2_plan_on_the_host(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "rdm2_host_check")
    static = ["-static-libsan"] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
                          + static + [os.path.join(HERE, "rdm2_host_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in PROPERTIES:
        assert "ok " + name in r.stdout, (name, r.stdout)
    assert "all ok" in r.stdout
