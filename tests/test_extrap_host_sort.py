"""sqmc_amd/csrc/host_sort.h, the library's restatement of the reference's shell sort by magnitude, against the independent model of
tests/extrap_checker.py: tests/extrap_sort_check.cpp, a stand-alone program built with the host compiler under the address and
undefined-behaviour sanitizers and run as a child.  No GPU, and nothing loaded into this process."""
import os
import shutil
import subprocess

import numpy as np

import extrap_checker as EC

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = (0, 1, 2, 3, 10, 11, 23, 1000)


def _cases():
    out = []
    for n in SIZES:
        rng = np.random.default_rng(100 + n)
        x = rng.standard_normal(n)
        neg = x.copy()
        if n:
            neg[int(np.argmax(np.abs(neg)))] = -abs(neg).max() - 1.0            # the leading element is negative: the sign flip
        by_mag = x[np.argsort(-np.abs(x), kind="stable")]
        out += [("all equal", np.full(n, -0.75)), ("three values", rng.choice([-1.0, 0.5, 1.0], n)), ("negative leader", neg),
                ("sorted", by_mag), ("reversed", by_mag[::-1].copy()), ("random", x), ("zeros", np.zeros(n))]
    return out


def test_host_sort_against_the_checker(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "extrap_sort_check")
    static = ["-static-libsan"] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
                          + static + [os.path.join(HERE, "extrap_sort_check.cpp"), "-o", exe])
    cases = _cases()
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as f:
        for _, a in cases:
            f.write("%d\n%s\n" % (len(a), " ".join(float(v).hex() for v in a)))
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    assert lines[3 * len(cases)] == "all ok %d" % len(cases)
    for k, (tag, a) in enumerate(cases):
        n = int(lines[3 * k])
        got = [float.fromhex(t) for t in lines[3 * k + 1].split()]
        order = [int(t) for t in lines[3 * k + 2].split()]
        want, want_order = EC.shell_sort_magnitude(a)
        assert n == len(a) and order == want_order, (tag, n)
        assert np.array(got).tobytes() == np.array(want).tobytes(), (tag, n)          # bits: -0.0 where the sign flip makes it
