#!/bin/bash
# Value-only mutants of the f16 accumulate producer / consumer: does tests/test_gpu_acc16_edges.py notice a wrong kernel?
#   tools/acc16_mutants.sh build [NAME ...]   HERE (hipcc cross-compiles; `make -C poccala_amd/csrc` first, the other objects are linked as they are):
#                                  for every mutant a copy of gmm_accumulate_f16.hip with ONE substitution (it must match exactly once) under
#                                  build_ab/acc16_mut_NAME/, compiled and linked -> build_ab/libpoccala_acc16_NAME.so
#   tools/acc16_mutants.sh run     on the GPU box: the shipped library must pass, then every mutant (POCCALA_HIP_LIB) must FAIL the file.  One
#                                  pytest call per mutant under its own timeout; any exit other than "passed" / "tests failed" stops the run.
# A mutant changes a value: a count that stays below the true one, a register <-> frame map, a row inside the accumulator, a scale, a store
# for an add, a coefficient, a factor.  No address leaves its buffer, every wait and barrier stays where it is.
set -e
cd "$(dirname "$0")/.."
SRC=poccala_amd/csrc/gmm_accumulate_f16.hip
NAMES="nf_clamp cf_order s0_row delta_no_gset rescale_no_gset fresh_store masked_left_in alpha_per_slice"
from_of() {
  case $1 in
    nf_clamp)        echo '(int)min(32LL, off[seg_hi[w]] - f0);' ;;
    cf_order)        echo 'r = q & 15, f = (r & 3) + 8 * (r >> 2) + 4 * h;' ;;
    s0_row)          echo 'constexpr int C0 = ((KS - 1) & 1) * 16 + (D & 7),' ;;
    delta_no_gset)   echo '__builtin_ceilf(rel) - G_SET' ;;
    rescale_no_gset) echo '__builtin_amdgcn_exp2f(-delta);' ;;
    fresh_store)     echo 'st_mean[o] += vm;' ;;
    masked_left_in)  echo '? -INFINITY : cfs[f];' ;;
    alpha_per_slice) echo 'if (lane == 0) st_alpha[j] += v;' ;;
  esac
}
to_of() {
  case $1 in
    nf_clamp)        echo '(int)min(32LL, off[seg_hi[w]] - f0 - 1);' ;;            # the last frame of every state is left out
    cf_order)        echo 'r = q & 15, f = (r & 3) + 8 * (r >> 2) + 4 * (1 - h);' ;;   # the lane halves swapped
    s0_row)          echo 'constexpr int C0 = ((KS - 1) & 1) * 16 + (D & 7) + 1,' ;;
    delta_no_gset)   echo '__builtin_ceilf(rel)' ;;                              # the scale 12 octaves higher: posteriors below 2^-24 of a mixture's largest are lost
    rescale_no_gset) echo '__builtin_amdgcn_exp2f(-(delta > 0.f ? delta + G_SET : delta));' ;;   # the sums rescaled by 2^-ceil(rel) while E moves by delta
    fresh_store)     echo 'st_mean[o] = vm;' ;;                                   # the read-modify-write flush stores
    masked_left_in)  echo '? cfs[f] : cfs[f];' ;;                                 # masked frames counted by both kernels
    alpha_per_slice) echo 'if (lane == 0) st_alpha[j] += v * (double)min(nslice, 2);' ;;   # what slice 1 adding gamma as well comes to
  esac
}
case $1 in
build)
  ls poccala_amd/csrc/pcl_api.o > /dev/null || { echo "make -C poccala_amd/csrc first"; exit 1; }
  OBJS=$(ls poccala_amd/csrc/*.o | grep -v gmm_accumulate_f16.o)
  shift
  for name in ${@:-$NAMES}; do
    mkdir -p build_ab/acc16_mut_$name
    FROM="$(from_of $name)" TO="$(to_of $name)" python3 - $SRC build_ab/acc16_mut_$name/gmm_accumulate_f16.hip <<'PY'
import os, sys
text = open(sys.argv[1]).read()
a, b = os.environ['FROM'], os.environ['TO']
assert text.count(a) == 1, '%r matches %d times' % (a, text.count(a))
open(sys.argv[2], 'w').write(text.replace(a, b))
PY
    /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC -fvisibility=hidden --offload-arch=gfx950 -Wno-unused-function -Wno-unused-value -Wno-unused-result \
      -Ipoccala_amd/csrc -c build_ab/acc16_mut_$name/gmm_accumulate_f16.hip -o build_ab/acc16_mut_$name/gmm_accumulate_f16.o
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o build_ab/libpoccala_acc16_$name.so $OBJS build_ab/acc16_mut_$name/gmm_accumulate_f16.o \
      -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib
    echo build_ab/libpoccala_acc16_$name.so
  done ;;
run)
  run_one() {                       # 0: passed, 1: tests failed; anything else ends the run
    set +e
    if [ -n "$1" ]; then POCCALA_HIP_LIB=$1 timeout -k 10 300 python3 -m pytest tests/test_gpu_acc16_edges.py -m gpu -q -p no:cacheprovider > "$2" 2>&1
    else timeout -k 10 300 python3 -m pytest tests/test_gpu_acc16_edges.py -m gpu -q -p no:cacheprovider > "$2" 2>&1; fi
    rc=$?
    set -e
    if [ $rc != 0 ] && [ $rc != 1 ]; then echo "ABNORMAL exit $rc ($2): nothing more is run"; tail -20 "$2"; exit 2; fi
    return 0
  }
  out=${ACC16_OUT:-build_ab}
  mkdir -p $out
  run_one "" $out/acc16_mutant_shipped.log
  [ $rc = 0 ] || { echo "the shipped library does not pass"; tail -30 $out/acc16_mutant_shipped.log; exit 1; }
  echo "shipped: passes ($(tail -1 $out/acc16_mutant_shipped.log))"
  survived=0
  for name in $NAMES; do
    [ -f build_ab/libpoccala_acc16_$name.so ] || { echo "build_ab/libpoccala_acc16_$name.so is missing: tools/acc16_mutants.sh build"; exit 1; }
    run_one $PWD/build_ab/libpoccala_acc16_$name.so $out/acc16_mutant_$name.log
    if [ $rc = 1 ]; then echo "$name: CAUGHT  $(grep -c '^FAILED' $out/acc16_mutant_$name.log) tests fail: $(grep '^FAILED' $out/acc16_mutant_$name.log | sed 's/ - .*//; s/.*:://' | tr '\n' ' ' | cut -c1-600)"
    else echo "$name: SURVIVED"; survived=1; fi
  done
  exit $survived ;;
*) echo "usage: $0 build|run"; exit 2 ;;
esac
