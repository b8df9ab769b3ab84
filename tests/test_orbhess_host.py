"""The host arithmetic of the one-index transformation (sqmc_amd/csrc/orbopt_plan.h: the pairs, the symmetrising tiles and their owners,
the register-tile switch, the sizes that must fit): tests/orbhess_host_check.cpp, a stand-alone program built with the host compiler
under the address and undefined-behaviour sanitizers and run as a child."""
import os
import shutil
import subprocess


HERE = os.path.dirname(os.path.abspath(__file__))
PROPERTIES = ["shapes of every size", "one owner per packed entry", "pair numbering"]


def test_orbhess_plan_on_the_host(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "orbhess_host_check")
    static = ["-static-libsan"] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
                          + static + [os.path.join(HERE, "orbhess_host_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in PROPERTIES:
        assert "ok " + name in r.stdout, (name, r.stdout)
    assert "all ok" in r.stdout
