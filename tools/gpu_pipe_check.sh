cd $GRAFT_REPO_ROOT
O=${1:?usage: gpu_pipe_check.sh OUTPUT_DIR}/pipe; mkdir -p $O
timeout 900 python -m pytest tests/test_gpu_units.py -x -q -W ignore -k "exchange or rccl or mstep or em_loop" 2>&1 | tail -8 | tee $O/tests.log
timeout 600 python bench.py --full --cpu-baseline 0 > $O/bench.json 2> $O/bench.err; tail -3 $O/bench.err
python - $O/bench.json <<'P'
import json, sys
d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
e=d['extra']
print('value', d['value'], 'estep_ms', e['estep_ms'], 'acc', e['accumulate_ms'])
print('exchange', e['exchange']['per_rank'])
print('pipe', e.get('estep_pipelined'))
print('err', e.get('error'))
P
