O=${1:?usage: $0 <output directory>}; mkdir -p $O
python -m pytest tests -m gpu -x -q > $O/pytest_gpu.log 2>&1; tail -2 $O/pytest_gpu.log | head -1
python bench.py --full --config c2 --timed-events none --no-cpu-baseline > $O/c2.json 2> $O/c2.err
python bench.py --full --config c3 --timed-events none --no-cpu-baseline > $O/c3.json 2> $O/c3.err
python bench.py --full --rows 125000 --no-cpu-baseline > $O/c4_shard125k.json 2> $O/c4_shard125k.err
python bench.py --full --no-cpu-baseline > $O/c4.json 2> $O/c4.err
for f in c2 c3 c4_shard125k c4; do python -c "
import json,sys; d=json.loads(open('$O/$f.json').read().strip().splitlines()[-1]); s=d['kernels']['stage_ms_per_eval']; print('$f', d['value'], d['ms_per_step'], 'row_scalars', s['row_scalars'], 'solve_vectors', s['solve_vectors'])"; done
