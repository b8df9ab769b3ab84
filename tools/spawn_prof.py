#!/usr/bin/env python3
"""Where the time of k_spawn goes at the bench size: rebuilds the library with -DSPAWN_PROF on the GPU box, runs the bench
configuration and prints, per phase, the mean / max over the spawning blocks of the last step (wall clock, 100 MHz ticks), then
the spare blocks in front of them by kind: how many, how long they live, when the last of each kind ends after the kernel's first
stamp -- beside the end of the last spawning block -- and the phases of the bucket-boundary block(s).
The instrumented build is a file of its own (sqmc_amd/_lib.py: the flags are part of its name); the product's library is not touched."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["SQMC_EXTRA_CFLAGS"] = "-DSPAWN_PROF"
import torch  # noqa: F401
import sqmc_amd
sqmc_amd.build_library()
from sqmc_amd import host as H

target = float(sys.argv[1]) if len(sys.argv) > 1 else 1e5
hst = H.ChemHost(os.path.join(ROOT, "tests", "golden", "C2_r1.24253_FCIDUMP"), 8, 4, "d2h")
w = H.GpuWalk(hst, target, seed=(1346, 5634, 6635, 4361), w_begin=min(target, 1e4))
w.run(500 if target <= 2e5 else 1200, keep_stats=False)
L = sqmc_amd.load_library()
buf = (C.c_uint64 * (8 * 8192))()
assert L.sqmc_gpu_debug_prof(buf) == 0
old = np.array(buf, dtype=np.int64).reshape(8192, 8)
w.run(2, keep_stats=False)
assert L.sqmc_gpu_debug_prof(buf) == 0
a = np.array(buf, dtype=np.int64).reshape(8192, 8)
live = (a[:, 5] != old[:, 5]) & (a[:, 5] > a[:, 0])           # blocks that spawned in the last step (stamp 5 = end)
allb = a[live]
a = allb[allb[:, 6] == 0]                                    # stamp 6 = kind of block: 0 spawning, 1.. the spare blocks (bucket_partition.h)
t0 = a[:, 0].min()
print("tail stats", w.g.tail_stats(), "spawning blocks", len(a), "kernel span %.1f us" % ((a[:, 5].max() - t0) / 100.0))
print("start skew: mean %.1f max %.1f us" % ((a[:, 0] - t0).mean() / 100.0, (a[:, 0] - t0).max() / 100.0))
late = (a[:, 0] - t0) > 200                                   # more blocks than the chip holds at once: these waited for another block to end
print("spawning blocks that start more than 2 us after the first: %d (their start: mean %.1f us)" % (late.sum(), (a[late, 0] - t0).mean() / 100.0 if late.any() else 0.0))
names = ["table staging + first probe + splitters", "parent window (256-way probes + LDS window)", "parent search + loads", "proposal", "weight + emit", "partition (bucket search, ranks, offsets, words)"]
for k in range(1, 6):
    d = (a[:, k] - a[:, k - 1]) / 100.0
    print("%-52s mean %6.2f  max %6.2f us" % (names[k - 1] if k < 5 else names[5], d.mean(), d.max()))
d = (a[:, 5] - a[:, 0]) / 100.0
print("block life: mean %.1f max %.1f us" % (d.mean(), d.max()))
k0 = allb[:, 0].min()                                        # the kernel's first stamp (a spare block's: they lead the grid)
print("spare blocks of the same launch, times after the kernel's first stamp (%.1f us before the first spawning block's):" % ((t0 - k0) / 100.0))
kinds = ["spawning", "final sums", "H_ii queue", "projector rows", "boundaries" + (": positions" if (allb[:, 6] == 5).any() else ""), "boundaries: next"]
for kd in (1, 2, 3, 4, 5, 0):
    b = allb[allb[:, 6] == kd]
    if len(b) == 0:
        continue
    d = (b[:, 5] - b[:, 0]) / 100.0
    print("%-24s n %5d  life mean %6.2f  max %6.2f us  last start %6.2f  last end %6.2f us" % (kinds[kd], len(b), d.mean(), d.max(), (b[:, 0].max() - k0) / 100.0,
                                                                                          (b[:, 5].max() - k0) / 100.0))
for kd in (4, 5):
    for b in allb[allb[:, 6] == kd]:
        st = [int(b[0])] + [int(b[k]) for k in (1, 2, 3) if b[k] > b[0]] + [int(b[5])]      # stamps this block took (a block without next boundaries takes none inside)
        if len(st) == 5:
            ph = ["position search" if kd == 4 and not (allb[:, 6] == 5).any() else "loads + terms", "serial sum", "second search", "validation + stores"]
            print("%-24s " % kinds[kd] + "  ".join("%s %.2f" % (ph[k], (st[k + 1] - st[k]) / 100.0) for k in range(4)) + " us")
last_spare = allb[allb[:, 6] != 0][:, 5].max() if (allb[:, 6] != 0).any() else k0
print("kernel ends with its %s blocks: last spare block %.2f us, last spawning block %.2f us after the first stamp" % (
    "spare" if last_spare > a[:, 5].max() else "spawning", (last_spare - k0) / 100.0, (a[:, 5].max() - k0) / 100.0))
w.close()
