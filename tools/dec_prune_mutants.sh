#!/bin/bash
# Value-only mutants of the decoders' pruning / transfer helpers: does tests/test_gpu_dec_prune.py notice a wrong helper?
#   tools/dec_prune_mutants.sh build   HERE (hipcc cross-compiles): for every mutant, a copy of hmm_decode_common.h with ONE substitution
#                                      (it must match exactly once) under build_ab/dec_mut_NAME/, and the harness built against the
#                                      copy -> build_ab/libdectest_NAME.so
#   tools/dec_prune_mutants.sh run     on the GPU box: the shipped harness must pass, then every mutant must FAIL the test
#                                      (DECTEST_LIB selects the library).  One pytest call per mutant under its own timeout; any exit
#                                      other than "passed" / "tests failed" stops the run.
# A mutant changes a comparison or a tie-break, never an index, a loop bound, a barrier or an allocation size.
set -e
cd "$(dirname "$0")/.."
HDR=poccala_amd/csrc/hmm_decode_common.h
NAMES="select_bin_le mark_lt_rank distinct_ge beats_later hist_not_rezeroed cand_less_lt"
from_of() {
  case $1 in
    select_bin_le)     echo 'rank < lo + s4' ;;
    mark_lt_rank)      echo '__popcll(mask & lt_mask) <= rank' ;;
    distinct_ge)       echo 'key > prev' ;;
    beats_later)       echo 'oi < bi' ;;
    hist_not_rezeroed) echo 'if (scans) hist[BPT * tid + j] = 0u;' ;;
    cand_less_lt)      echo 'less <= rank' ;;
  esac
}
to_of() {
  case $1 in
    select_bin_le)     echo 'rank <= lo + s4' ;;
    mark_lt_rank)      echo '__popcll(mask & lt_mask) < rank' ;;
    distinct_ge)       echo 'key >= prev' ;;
    beats_later)       echo 'oi > bi' ;;
    hist_not_rezeroed) echo '(void)0;' ;;
    cand_less_lt)      echo 'less < rank' ;;
  esac
}
case $1 in
build)
  for name in $NAMES; do
    mkdir -p build_ab/dec_mut_$name
    FROM="$(from_of $name)" TO="$(to_of $name)" python3 - $HDR build_ab/dec_mut_$name/hmm_decode_common.h <<'PY'
import os, sys
text = open(sys.argv[1]).read()
a, b = os.environ['FROM'], os.environ['TO']
assert text.count(a) == 1, '%r matches %d times' % (a, text.count(a))
open(sys.argv[2], 'w').write(text.replace(a, b))
PY
    /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC -fvisibility=hidden --offload-arch=gfx950 -Wno-unused-value -Wno-unused-result \
      -Ibuild_ab/dec_mut_$name -Ipoccala_amd/csrc -shared -o build_ab/libdectest_$name.so tests/dec_prune_harness.hip -L/opt/rocm/lib -Wl,-rpath,/opt/rocm/lib
    echo build_ab/libdectest_$name.so
  done ;;
run)
  run_one() {                       # 0: passed, 1: tests failed; anything else ends the run
    set +e
    DECTEST_LIB=$1 timeout -k 10 300 python3 -m pytest tests/test_gpu_dec_prune.py -m gpu -q -p no:cacheprovider > "$2" 2>&1
    rc=$?
    set -e
    if [ $rc != 0 ] && [ $rc != 1 ]; then echo "ABNORMAL exit $rc ($2): nothing more is run"; tail -20 "$2"; exit 2; fi
    return 0
  }
  out=${DECTEST_OUT:-build_ab}
  mkdir -p $out
  run_one "" $out/mutant_shipped.log
  [ $rc = 0 ] || { echo "the shipped harness does not pass"; tail -30 $out/mutant_shipped.log; exit 1; }
  echo "shipped: passes"
  survived=0
  for name in $NAMES; do
    [ -f build_ab/libdectest_$name.so ] || { echo "build_ab/libdectest_$name.so is missing: tools/dec_prune_mutants.sh build"; exit 1; }
    run_one $PWD/build_ab/libdectest_$name.so $out/mutant_$name.log
    if [ $rc = 1 ]; then echo "$name: CAUGHT  $(grep -c '^FAILED' $out/mutant_$name.log) tests fail: $(grep '^FAILED' $out/mutant_$name.log | sed 's/ - .*//; s/.*:://' | tr '\n' ' ')"
    else echo "$name: SURVIVED"; survived=1; fi
  done
  exit $survived ;;
*) echo "usage: $0 build|run"; exit 2 ;;
esac
