#!/bin/bash
# Value-only mutants of segmental training (counting sort, seeding, Lloyd, cluster model, M-step + Q): does tests/test_gpu_segment_edges.py
# notice a wrong kernel?
#   tools/seg_mutants.sh build [NAME ...]   HERE (hipcc cross-compiles; `make -C poccala_amd/csrc` first, the other objects are linked as they are):
#                                  for every mutant a copy of gmm_segment.hip with ONE substitution (it must match exactly once) under
#                                  build_ab/seg_mut_NAME/, compiled and linked -> build_ab/libpoccala_seg_NAME.so
#   tools/seg_mutants.sh run       on the GPU box: the shipped library must pass, then every mutant (POCCALA_HIP_LIB) must FAIL the file.  One
#                                  pytest call per mutant under its own timeout; any exit other than "passed" / "tests failed" stops the run.
# A mutant changes a value: an index that stays inside its chunk, a comparison, a count that stays below the true one, a floor, a prefix, a
# rank that is still a permutation, a loop bound below the true one, a term, a constant.  No address leaves its buffer, every wait and
# barrier stays where it is.
set -e
cd "$(dirname "$0")/.."
SRC=poccala_amd/csrc/gmm_segment.hip
NAMES="chunk_index tie_highest quarter_floor var_floor seed_prefix round_rank mix_bound s2_about_old logdet_arms"
from_of() {
  case $1 in
    chunk_index)   echo 'bk = k0 + kk;' ;;
    tie_highest)   echo 'if (acc < best) {' ;;
    quarter_floor) echo 'const int q = (cnt + 3) / 4,' ;;
    var_floor)     echo 'if (!(v >= 1e-4)) v = 1e-4;' ;;
    seed_prefix)   echo 'part[t] = run;' ;;
    round_rank)    echo 'rank += same & (t < (int)threadIdx.x);' ;;
    mix_bound)     echo 'for (int m = threadIdx.x; m < M; m += SEG_T) {' ;;
    s2_about_old)  echo 'double s2 = st_cov[i] / g - (mu - c) * (mu - c);' ;;
    logdet_arms)   echo '(logdet ? log(v) : v)' ;;
  esac
}
to_of() {
  case $1 in
    chunk_index)   echo 'bk = kk;' ;;                                             # the index inside the chunk for the centre's
    tie_highest)   echo 'if (acc <= best) {' ;;                                   # the highest index wins a tie
    quarter_floor) echo 'const int q = cnt / 4,' ;;                               # the tail rows of a cluster dropped (bounds still clamp to cnt)
    var_floor)     echo 'if (!(v >= 1e-6)) v = 1e-6;' ;;
    seed_prefix)   echo 'part[t] = run + v;' ;;                                   # the exclusive prefix of the seed draw made inclusive
    round_rank)    echo 'rank += same & (t > (int)threadIdx.x);' ;;               # the order inside a 256-row round reversed: still a permutation
    mix_bound)     echo 'for (int m = threadIdx.x; m < min(M, 256); m += SEG_T) {' ;;   # mixtures from 256 on keep what they had
    s2_about_old)  echo 'double s2 = st_cov[i] / g;' ;;                           # the variance about the OLD mean
    logdet_arms)   echo '(logdet ? v : log(v))' ;;
  esac
}
case $1 in
build)
  ls poccala_amd/csrc/pcl_api.o > /dev/null || { echo "make -C poccala_amd/csrc first"; exit 1; }
  OBJS=$(ls poccala_amd/csrc/*.o | grep -v gmm_segment.o)
  shift
  for name in ${@:-$NAMES}; do
    mkdir -p build_ab/seg_mut_$name
    FROM="$(from_of $name)" TO="$(to_of $name)" python3 - $SRC build_ab/seg_mut_$name/gmm_segment.hip <<'PY'
import os, sys
text = open(sys.argv[1]).read()
a, b = os.environ['FROM'], os.environ['TO']
assert text.count(a) == 1, '%r matches %d times' % (a, text.count(a))
open(sys.argv[2], 'w').write(text.replace(a, b))
PY
    /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC -fvisibility=hidden --offload-arch=gfx950 -Wno-unused-function -Wno-unused-value -Wno-unused-result \
      -Ipoccala_amd/csrc -c build_ab/seg_mut_$name/gmm_segment.hip -o build_ab/seg_mut_$name/gmm_segment.o
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o build_ab/libpoccala_seg_$name.so $OBJS build_ab/seg_mut_$name/gmm_segment.o \
      -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib
    echo build_ab/libpoccala_seg_$name.so
  done ;;
run)
  run_one() {                       # 0: passed, 1: tests failed; anything else ends the run
    set +e
    if [ -n "$1" ]; then POCCALA_HIP_LIB=$1 timeout -k 10 300 python3 -m pytest tests/test_gpu_segment_edges.py -m gpu -q -p no:cacheprovider > "$2" 2>&1
    else timeout -k 10 300 python3 -m pytest tests/test_gpu_segment_edges.py -m gpu -q -p no:cacheprovider > "$2" 2>&1; fi
    rc=$?
    set -e
    if [ $rc != 0 ] && [ $rc != 1 ]; then echo "ABNORMAL exit $rc ($2): nothing more is run"; tail -20 "$2"; exit 2; fi
    return 0
  }
  out=${SEG_OUT:-build_ab}
  mkdir -p $out
  run_one "" $out/seg_mutant_shipped.log
  [ $rc = 0 ] || { echo "the shipped library does not pass"; tail -30 $out/seg_mutant_shipped.log; exit 1; }
  echo "shipped: passes ($(tail -1 $out/seg_mutant_shipped.log))"
  survived=0
  for name in $NAMES; do
    [ -f build_ab/libpoccala_seg_$name.so ] || { echo "build_ab/libpoccala_seg_$name.so is missing: tools/seg_mutants.sh build"; exit 1; }
    run_one $PWD/build_ab/libpoccala_seg_$name.so $out/seg_mutant_$name.log
    if [ $rc = 1 ]; then echo "$name: CAUGHT  $(grep -c '^FAILED' $out/seg_mutant_$name.log) tests fail: $(grep '^FAILED' $out/seg_mutant_$name.log | sed 's/ - .*//; s/.*:://' | tr '\n' ' ' | cut -c1-600)"
    else echo "$name: SURVIVED"; survived=1; fi
  done
  exit $survived ;;
*) echo "usage: $0 build|run"; exit 2 ;;
esac
