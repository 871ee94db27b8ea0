#!/bin/bash
# k_fast_strips cut after a prefix of its stages (-DORBX_FAST_CUT=0/1/2/3: after the tile load, after stage 1, after stage 2, after the whole iniThFAST pass): the
# stage time of each variant tells what the stages cost in the full kernel; "full" minus cut 3 is the share of the minThFAST fallback cells.  Results of the cut
# variants are wrong by construction.
# usage (repo root, after `make -C orb_slam3-1_amd/csrc`):  bash tools/fast_cuts.sh [build|run]
#   build  compiles the variants into $CUT_DIR (default /tmp/orbx_cuts; needs the object files of the make, no GPU)
#   run    times every variant found in $CUT_DIR and the full library (GPU box); without an argument: both
CUT_DIR=${CUT_DIR:-/tmp/orbx_cuts}
LIB=orb_slam3-1_amd/liborbslam3_hip.so
mode=${1:-both}
mkdir -p "$CUT_DIR"
if [ "$mode" != run ]; then
  others=$(ls orb_slam3-1_amd/csrc/*.o | grep -v orbx_extractor.o)
  for v in 0 1 2 3; do
    /opt/rocm/bin/hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -fPIC -std=c++17 -DORBX_FAST_CUT=$v -c -o "$CUT_DIR/ex_cut$v.o" orb_slam3-1_amd/csrc/orbx_extractor.hip &&
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$CUT_DIR/lib_cut$v.so" $others "$CUT_DIR/ex_cut$v.o" && rm -f "$CUT_DIR/ex_cut$v.o" || exit 1
  done
fi
[ "$mode" = build ] && exit 0
cp $LIB "$CUT_DIR/lib_full.so"
# whatever happens (a timeout, an interrupt): the full library comes back
trap 'cp "$CUT_DIR/lib_full.so" $LIB' EXIT
for v in 0 1 2 3 full; do
  [ -f "$CUT_DIR/lib_cut$v.so" ] || [ $v = full ] || continue
  [ $v = full ] || cp "$CUT_DIR/lib_cut$v.so" $LIB
  [ $v = full ] && cp "$CUT_DIR/lib_full.so" $LIB
  timeout -k 10 120 python - <<PY || exit 1
import importlib, numpy as np, torch, sys
sys.path.insert(0, ".")
pkg = importlib.import_module("orb_slam3-1_amd"); synth = importlib.import_module("orb_slam3-1_amd.synth")
ex = pkg.Extractor(); ex.profile_enable(True)
imgs = np.stack([synth.make_frame(i) for i in range(16)] * 16)
for rep in range(3):
    try:
        ex.extract_batch(imgs)
    except Exception as e:
        pass
print("cut $v:", ex.profile_read())
PY
done
