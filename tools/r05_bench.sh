O=${1:?usage: $0 <output directory>}; mkdir -p $O
python bench.py --full > $O/c4.json 2> $O/c4.err; tail -c 2500 $O/c4.json; tail -3 $O/c4.err
python bench.py --full --config c2 --no-cpu-baseline > $O/c2.json 2> $O/c2.err; python -c "
import json; d=json.loads(open('$O/c2.json').read().strip().splitlines()[-1]); print('c2', d['value'], d['ms_per_step'], d['stage_pass'], d['route'])"
python bench.py --full --native-mgpu 8 --no-cpu-baseline --steps 5 > $O/c4_mgpu8.json 2> $O/c4_mgpu8.err; python -c "
import json; d=json.loads(open('$O/c4_mgpu8.json').read().strip().splitlines()[-1]); print('mgpu8', d['value'], d['ms_per_step'], d['stage_pass'], d['per_rank'][0]['route'], d['per_rank'][1])"; tail -3 $O/c4_mgpu8.err
python bench.py --full --rows 125000 --no-cpu-baseline > $O/c4_shard125k.json 2>$O/c4_shard125k.err;  python -c "
import json; d=json.loads(open('$O/c4_shard125k.json').read().strip().splitlines()[-1]); print('shard125k', d['value'], d['ms_per_step'], d['stage_pass'])"
