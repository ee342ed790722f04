#!/bin/bash
# Does averaging the generator's weights (--ema_decay) narrow the seed-to-seed
# scatter of what a run ends with?  BASELINE configs[1] end to end, as
# tools/e2e_seeds.sh runs it: main.py for EPOCHS epochs on the DG set, the
# generated set of the last epoch through compute_dg_metrics.py, per seed of the
# noise / interpolation / shift streams (CALCIUMGAN_SEED) two arms:
#   raw   no flag: the weights the last Adam step left
#   ema   --ema_decay $DECAY: the same training trajectory bit for bit
#         (tests/test_hip_ema.py), validated and sampled from the average
# so the arms are PAIRED by seed.  One line per run, then per arm mean, sd and
# worst seed of firing-rate MAE and covariance MAE, and the paired differences.
# Every GPU step runs once under its own time limit; a failure ends the script.
# BUDGET_S (optional): no further seed is started once the time used plus the
# time the slowest seed so far took would pass it; the summary says how many ran.
set -u
D=/tmp/dg2048; O=${OUT:-runs/e2e_ema}; mkdir -p $O
EPOCHS=${EPOCHS:-100}
DECAY=${DECAY:-0.999}
T0=$SECONDS
if [ ! -d $D ]; then
timeout -k 10 900 python dataset/generate_dg_dataset.py --output_dir $D --sequence_length 2048 \
  --num_neurons 102 --num_segments 9192 --validation_size 1000 > $O/dataset.log 2>&1 || exit 1
fi
: > $O/runs.txt
slowest=0
for seed in ${SEEDS:-1 2 3 4 5 6 7}; do
  if [ -n "${BUDGET_S:-}" ] && [ $((SECONDS - T0 + slowest)) -gt $BUDGET_S ]; then
    echo "(seed $seed and later not started: time budget)" | tee -a $O/runs.txt
    break
  fi
  s0=$SECONDS
  for arm in raw ema; do
    R=/tmp/run_${arm}_$seed
    flag=; [ $arm = ema ] && flag="--ema_decay $DECAY"
    CALCIUMGAN_SEED=$seed timeout -k 10 ${TRAIN_LIMIT_S:-600} python main.py --input_dir $D --output_dir $R \
      --model calciumgan --algorithm wgan-gp --batch_size 128 --num_units 64 --kernel_size 24 \
      --strides 2 --m 10 --layer_norm --epochs $EPOCHS --save_generated last --skip_checkpoints \
      --clear_output_dir --verbose 0 $flag > $O/train_${arm}_$seed.log 2>&1 || exit 1
    CALCIUMGAN_METRICS_JSON=$O/metrics_${arm}_$seed.json timeout -k 10 ${METRICS_LIMIT_S:-400} python compute_dg_metrics.py \
      --output_dir $R --num_trials ${TRIALS:-200} > $O/metrics_${arm}_$seed.log 2>&1 || exit 1
    python3 - $arm $seed $O/metrics_${arm}_$seed.json $R/scalars.jsonl <<'PY' | tee -a $O/runs.txt
import json, sys
arm, seed, mj, sj = sys.argv[1:5]
m = json.load(open(mj))
last = {}
for l in open(sj):
  r = json.loads(l)
  last[r['tag']] = r['value']
print('%-3s seed %s  firing rate MAE %.4f RMSE %.4f  covariance MAE %.5f  population rate fake %.4f real %.4f  cov fake %.5f real %.5f  | last epoch: G %.2f D %.2f gp %.3f  %.0f samples/s' % (
    arm, seed, m['firing_rate']['mae'], m['firing_rate']['rmse'], m['covariance']['mae'],
    m['population']['fake_rate'], m['population']['real_rate'], m['population']['fake_cov'],
    m['population']['real_cov'], last.get('loss/generator', 0), last.get('loss/discriminator', 0),
    last.get('loss/gradient_penalty', 0), last.get('samples_per_sec', 0)), flush=True)
PY
  done
  took=$((SECONDS - s0)); [ $took -gt $slowest ] && slowest=$took
done
python3 - $O $EPOCHS $DECAY <<'PY' | tee $O/summary.txt
import glob, json, os, re, statistics as st, sys
O, epochs, decay = sys.argv[1:4]
runs = {}
for f in glob.glob(os.path.join(O, 'metrics_*_*.json')):
  arm, seed = re.match(r'metrics_(raw|ema)_(\d+)\.json', os.path.basename(f)).groups()
  m = json.load(open(f))
  runs.setdefault(int(seed), {})[arm] = (m['firing_rate']['mae'], m['covariance']['mae'])
seeds = sorted(s for s, a in runs.items() if len(a) == 2)
print(open(os.path.join(O, 'runs.txt')).read().rstrip())
print()
print('seeds %s (n = %d per arm), %s epochs, --ema_decay %s' % (
    ' '.join(map(str, seeds)), len(seeds), epochs, decay))
sd = lambda v: st.stdev(v) if len(v) > 1 else float('nan')
for k, name, fmt in ((0, 'firing rate MAE', '%.4f'), (1, 'covariance MAE ', '%.5f')):
  cells = []
  for arm in ('raw', 'ema'):
    v = [runs[s][arm][k] for s in seeds]
    worst = max(seeds, key=lambda s: runs[s][arm][k])
    cells.append(('%s mean ' + fmt + ' sd ' + fmt + ' worst ' + fmt + ' (seed %d)') % (
        arm, st.mean(v), sd(v), runs[worst][arm][k], worst))
  d = [runs[s]['ema'][k] - runs[s]['raw'][k] for s in seeds]
  se = sd(d) / len(d) ** 0.5 if len(d) > 1 else float('nan')
  print(('  %s  %s | %s | paired ema - raw: mean ' + fmt.replace('%', '%+') + ' +- ' + fmt +
         ' (s.e.), ema lower in %d of %d; per seed ' + ' '.join([fmt.replace('%', '%+')] * len(d))) % (
             (name, cells[0], cells[1], st.mean(d), se, sum(x < 0 for x in d), len(d)) + tuple(d)))
PY
