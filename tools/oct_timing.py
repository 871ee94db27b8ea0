#!/usr/bin/env python3
"""Cycle split of the level-0 octree wave of one frame (GPU box).  Needs orbx_extractor.hip compiled with -DORBX_OCT_TIMING
(hipcc ... -DORBX_OCT_TIMING -c orbx_extractor.hip, then make; rebuild with `make -B` afterwards)."""
import ctypes as C
import importlib
import os
import sys

import torch  # noqa: F401

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("orb_slam3-1_amd")
synth = importlib.import_module("orb_slam3-1_amd.synth")
ex = pkg.Extractor()
img = synth.make_frame(0)
ex(img); ex(img)
out = (C.c_ulonglong * 11)()
pkg.lib.orbx_debug_oct_prof(out)
v = list(out)
# "placement": every key once to its cell of the bucket table (counting sort); "partition below the table": the count + scatter of the
# nodes deeper than the table (all the divides' key movement before the table existed: the bucket then read "count+scatter")
names = ["placement", "roots", "child sizes (lookup / partition below the table)", "bookkeeping", "compact/other", "sort", "final selection"]
print("level-0 wave: %d cycles, %d candidates, %d divides" % (v[7], v[8], v[9]))
print("  " + ", ".join("%s %d" % (n, c) for n, c in zip(names, v[:7])))
print("  waiting at the job barriers %d (control wave, %d waves per workgroup)" % (v[10], ex.debug_octree_waves(1)))
