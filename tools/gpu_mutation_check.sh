#!/bin/bash
# The mutation builds: the library with a known, fixed bug restored must FAIL the test that guards the fix.  Build them HERE first:
#   tools/build_variant.sh lseflush "-DPCL_LSE_FLUSH_REPRO -fno-slp-vectorize" gmm_score_split.hip gmm_score_mfma.hip
#   tools/build_variant.sh race "-DPCL_DESC_RACE_REPRO" pcl_batch.hip hmm_units.hip
#   tools/build_variant.sh coarsemargin "-DPCL_COARSE_MARGIN_REPRO" gmm_score_coarse.hip      (round 6: the coarse pass rules out pairs that matter)
#   tools/build_variant.sh coarselast "-DPCL_COARSE_LASTSTAGE_REPRO" gmm_score_coarse.hip      (a give-up in the coarse pass's last stage drops its tiles)
#   tools/build_variant.sh coarseclamp "-DPCL_COARSE_CLAMP_REPRO" gmm_score_coarse.hip         (pairs ruled out under a clamped threshold stand)
# then:  gpurun -- 'bash tools/gpu_mutation_check.sh'.  Exit code 0 = every mutant was caught (and the shipped library passes the same tests).
ROOT=$(cd "$(dirname "$0")/.." && pwd); cd "$ROOT"
OUT=${MUTATION_OUT:-build_ab/mutation}; mkdir -p "$OUT"      # (each run's pytest output)
rc=0
check() { # name, library, expected ("fail" / "pass"), pytest args...
  name=$1; lib=$2; want=$3; shift 3
  POCCALA_HIP_LIB=$lib timeout -k 10 400 python3 -m pytest "$@" -q > "$OUT"/mutation_$name.txt 2>&1; got=$?
  if [ "$want" = fail ] && [ $got -ne 0 ] && grep -q "failed" "$OUT"/mutation_$name.txt; then echo "$name: CAUGHT ($(tail -1 "$OUT"/mutation_$name.txt))";
  elif [ "$want" = pass ] && [ $got -eq 0 ]; then echo "$name: passes ($(tail -1 "$OUT"/mutation_$name.txt))";
  else echo "$name: UNEXPECTED rc=$got ($(tail -1 "$OUT"/mutation_$name.txt))"; rc=1; fi
}
L=$ROOT/poccala_amd/libpoccala_hip.so
check shipped_lse $L pass tests/test_gpu_parity.py -k "far_above_the_first_tile"
check mutant_lse $ROOT/build_ab/lib_lseflush.so fail tests/test_gpu_parity.py -k "far_above_the_first_tile"
check shipped_race $L pass tests/test_gpu_sweep.py
check mutant_race $ROOT/build_ab/lib_race.so fail tests/test_gpu_sweep.py
check shipped_coarse $L pass tests/test_gpu_coarse.py -k "six_decades or e_step"
check mutant_coarse $ROOT/build_ab/lib_coarsemargin.so fail tests/test_gpu_coarse.py -k "six_decades or e_step"
check shipped_coarselast $L pass tests/test_gpu_coarse.py -k "last_stage"
check mutant_coarselast $ROOT/build_ab/lib_coarselast.so fail tests/test_gpu_coarse.py -k "last_stage"
check shipped_coarseclamp $L pass tests/test_gpu_coarse.py -k "clamped_threshold"
check mutant_coarseclamp $ROOT/build_ab/lib_coarseclamp.so fail tests/test_gpu_coarse.py -k "clamped_threshold"
exit $rc
