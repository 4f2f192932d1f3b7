#!/bin/bash
# One entry point for every GPU-box task (run through gpurun from the repo root):
#
#   bash tools/gpu.sh tests [PYTEST_ARGS]     GPU test suite (one pytest process) + __graft_entry__.smoke()
#   bash tools/gpu.sh headline                driver-equivalent bench.py (STEPS=20 WARMUP=5 EXTRA= TAG=)
#   bash tools/gpu.sh timeline                kernel timeline of a population step (P=5 SAMPLES=2000 SPACE= KERNELS= BN=)
#   bash tools/gpu.sh prof NAME -- CMD...     rocprofv3 --kernel-trace --stats, keeps the stats CSVs
#   bash tools/gpu.sh pmc NAME "CTRS" -- CMD  one PMC pass (kernel-trace only) + tools/pmc_summary.py
#   bash tools/gpu.sh profstep                stats + 3 PMC passes of a population step -> tools/pmc_table.py (P= SPACE= KERNELS= BN= OUT=)
#   bash tools/gpu.sh conv                    conv microbench tools/bench_conv.py (GS="25" ONLY= DBGS=0), fp32 tests first
#   bash tools/gpu.sh ab                      tests + population-step A/B: ab_old/ (built previous tree) vs this tree
#   bash tools/gpu.sh qcurve                  groups per launch vs throughput, both fold protocols
#   bash tools/gpu.sh ga                      long RR-GA search with checkpoints (GENS= CKPT= BUDGET= GA_ARGS=)
#   bash tools/gpu.sh gbdt                    GBDT GPU tests, GA bench and kernel stats (POP= ROUNDS=)
#   bash tools/gpu.sh gbdt-predict            Booster.predict: GPU forest predictor vs the CPU predictor (ROWS= FEATURES= TREES= DEPTH= THREADS=)
#   bash tools/gpu.sh gbdt-shap               Booster.predict(pred_contribs=True): GPU SHAP kernel vs the CPU predictor (ROWS= FEATURES= TREES= DEPTH= THREADS=)
#   bash tools/gpu.sh gbdt-interactions       Booster.predict(pred_interactions=True): GPU kernel vs the CPU predictor (ROWS= FEATURES= TREES= DEPTH= THREADS= SPLITS=)
#   bash tools/gpu.sh cnn-predict             CnnClassifier.predict: HIP predictor at 32 / 256 rows per launch vs stock torch on the GPU (ROWS= REPS=)
#   bash tools/gpu.sh cnn-ensemble            CnnEnsemble.predict: one k-group launch set vs k predictors one by one vs stock torch; fit_ensemble vs k fits (ROWS= REPS= K= FIT_ROWS=)
#   bash tools/gpu.sh cnn-augment             TrainConfig.augment: step time off / on (and the parent tree in ab_old/), gt_augment's kernel time (GROUPS_LIST= REPS= PROF_GROUPS= OUT=)
#   bash tools/gpu.sh cnn-distill             soft targets: step time of the parent tree (ab_old/) / off / label_smoothing / a target table, the head kernels' time from a kernel trace run of its own, the distillation record (GROUPS_LIST= REPS= PROF_GROUPS= OUT= ACC=0)
#   bash tools/gpu.sh cnn-tta                 predict(tta=...): views and mean on the device vs V plain HIP predicts combined in numpy vs stock torch, classifier and k-ensemble (ROWS= FIT_ROWS= K= REPS= OUT=)
#   bash tools/gpu.sh cnn-occlusion           occlusion(): copies built and packed on the device vs occlusion_views in numpy + plain HIP predicts vs stock torch, classifier and k-ensemble (ROWS= FIT_ROWS= K= REPS= OUT= TIME=)
#   bash tools/gpu.sh cnn-gradcam             gradcam(): forward + gt_head_gradcam vs plain HIP predict (the floor) vs stock-torch autograd vs occlusion(patch=4), classifier and k-ensemble; the new kernels' device time by events and by a kernel trace run of its own (ROWS= OCC_ROWS= FIT_ROWS= K= REPS= OUT= TIME=)
#   bash tools/gpu.sh rehearse                2-rank torchrun bench on one GPU (gloo control plane)
#   bash tools/gpu.sh secondary               bench lines: reference fold semantics, torch comparator
#
# Every GPU step runs under its own `timeout -k 10`; steps are chained so the first failure ends the call.
set -o pipefail
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}" || exit 1
export GENTUN_NO_AUTOBUILD=1
mkdir -p gpurun_out
task=${1:-}; shift || true

heartbeat() {   # a line every 50 s under gpurun_out/ so a long step is not taken for a hang
  ( while sleep 50; do date >> gpurun_out/heartbeat; done ) & HB=$!
  trap 'kill $HB 2>/dev/null' EXIT
}

rocprof_env() { cd /tmp && export TMPDIR=/tmp && cd "${GRAFT_REPO_ROOT:-$OLDPWD}"; }

case "$task" in
tests)
  timeout -k 10 1000 python -u -m pytest -m gpu -x -v --timeout 300 --timeout-method thread tests/ "$@" \
    > gpurun_out/gpu_tests.log 2>&1; rc=$?
  grep -E "passed|failed|FAILED|Error" gpurun_out/gpu_tests.log | tail -8
  [ $rc -eq 0 ] || exit $rc
  timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > gpurun_out/smoke.log 2>&1; rc=$?
  tail -3 gpurun_out/smoke.log | cut -c1-400
  exit $rc ;;
headline)
  heartbeat; mkdir -p gpurun_out/headline
  timeout -k 10 ${TIME:-700} python3 -u bench.py --gpus 1 --steps ${STEPS:-20} --warmup ${WARMUP:-5} ${EXTRA:-} \
    > gpurun_out/headline/bench${TAG:-}.json 2> gpurun_out/headline/bench${TAG:-}.err; rc=$?
  tail -3 gpurun_out/headline/bench${TAG:-}.err; cat gpurun_out/headline/bench${TAG:-}.json
  exit $rc ;;
timeline)
  rocprof_env; mkdir -p gpurun_out/timeline; rm -rf /tmp/tl
  WARM=0 timeout -k 10 300 rocprofv3 --kernel-trace -d /tmp/tl -o run --output-format csv -- \
    python3 tools/probe_pop.py ${P:-5} ${P:-5} 1 1 ${SAMPLES:-2000} > gpurun_out/timeline/run${TAG:-}.log 2>&1 \
    || { tail -5 gpurun_out/timeline/run${TAG:-}.log; exit 1; }
  TIMELINE_DUMP=${DUMP:-1} python3 tools/timeline.py "$(find /tmp/tl -name "*kernel_trace.csv" | head -1)" > gpurun_out/timeline/summary${TAG:-}.txt
  head -30 gpurun_out/timeline/summary${TAG:-}.txt ;;
prof)
  name=$1; shift; shift
  rocprof_env; rm -rf /tmp/prof_$name; mkdir -p gpurun_out/prof_$name
  timeout -k 10 600 rocprofv3 --kernel-trace --stats -d /tmp/prof_$name -o run --output-format csv -- "$@" \
    > gpurun_out/prof_$name/run.log 2>&1 || { tail -5 gpurun_out/prof_$name/run.log; exit 1; }
  find /tmp/prof_$name -name "*stats.csv" -exec cp {} gpurun_out/prof_$name/ \;
  head -16 gpurun_out/prof_$name/run_kernel_stats.csv 2>/dev/null | cut -d, -f1-4 ;;
pmc)
  name=$1; counters=$2; shift 3
  rocprof_env; rm -rf /tmp/pmc_$name; mkdir -p gpurun_out/pmc_$name
  timeout -s KILL 120 rocprofv3 --kernel-trace --pmc $counters -d /tmp/pmc_$name -o run --output-format csv -- "$@" \
    > gpurun_out/pmc_$name/run.log 2>&1 || { tail -5 gpurun_out/pmc_$name/run.log; exit 1; }
  python3 tools/pmc_summary.py /tmp/pmc_$name > gpurun_out/pmc_$name/summary.txt
  head -30 gpurun_out/pmc_$name/summary.txt ;;
profstep)
  out=gpurun_out/${OUT:-profstep}; mkdir -p $out; rocprof_env; export WARM=0
  cmd="python3 tools/probe_pop.py ${P:-5} ${P:-5} 1 1 ${SAMPLES:-2000}"
  rm -rf /tmp/ps_stats
  timeout -k 10 240 rocprofv3 --kernel-trace --stats -d /tmp/ps_stats -o run --output-format csv -- $cmd \
    > $out/stats_run.log 2>&1 || { tail -5 $out/stats_run.log; exit 1; }
  find /tmp/ps_stats -name "*kernel_stats.csv" -exec cp {} $out/kernel_stats.csv \;
  i=0
  for ctr in "SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_LDS SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE GRBM_GUI_ACTIVE" \
             "SQ_INSTS_VALU SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_VALU_MFMA_BUSY_CYCLES SQ_WAIT_INST_LDS SQ_INSTS_SALU SQ_ACTIVE_INST_VMEM SQ_ACTIVE_INST_LDS GRBM_GUI_ACTIVE" \
             "TCC_EA0_RDREQ_sum TCC_EA0_WRREQ_sum TCC_HIT_sum TCC_MISS_sum GRBM_GUI_ACTIVE"; do
    i=$((i+1)); rm -rf /tmp/ps_pmc$i
    timeout -s KILL 120 rocprofv3 --kernel-trace --pmc $ctr -d /tmp/ps_pmc$i -o run --output-format csv -- $cmd \
      > $out/pmc$i.log 2>&1 || { tail -5 $out/pmc$i.log; exit 1; }
    python3 tools/pmc_summary.py /tmp/ps_pmc$i > $out/pmc$i.txt
  done
  python3 tools/pmc_table.py $out > $out/table.txt; head -24 $out/table.txt ;;
conv)
  timeout -k 10 300 python -u -m pytest tests/test_hip_fp32.py -x -q --timeout 120 --timeout-method thread \
    > gpurun_out/fp32_tests.log 2>&1 || { tail -30 gpurun_out/fp32_tests.log; exit 1; }
  tail -1 gpurun_out/fp32_tests.log
  : > gpurun_out/bench_conv${TAG:-}.log
  for G in ${GS:-25}; do
    G=$G DBGS=${DBGS:-0} ONLY="${ONLY:-}" timeout -k 10 300 python -u tools/bench_conv.py ${REPS:-10} \
      >> gpurun_out/bench_conv${TAG:-}.log 2>&1 || { tail -5 gpurun_out/bench_conv${TAG:-}.log; exit 1; }
  done
  cut -c1-160 gpurun_out/bench_conv${TAG:-}.log ;;
ab)
  if [ -z "${SKIP_TESTS:-}" ]; then
    timeout -k 10 600 python -u -m pytest -m gpu -x -q --timeout 300 --timeout-method thread ${AB_TESTS:-tests/test_hip_fp32.py tests/test_hip_kernels.py tests/test_hip_train.py} \
      > gpurun_out/ab_tests.log 2>&1 || { tail -40 gpurun_out/ab_tests.log; exit 1; }
    tail -1 gpurun_out/ab_tests.log
  fi
  for i in $(seq ${REPS:-3}); do
    (cd ab_old && timeout -k 10 200 python tools/probe_pop.py ${P:-5} ${P:-5} 1 ${EP:-1} 10000) > gpurun_out/ab_old_$i.log 2>&1 \
      || { tail -20 gpurun_out/ab_old_$i.log; exit 1; }
    timeout -k 10 200 python tools/probe_pop.py ${P:-5} ${P:-5} 1 ${EP:-1} 10000 > gpurun_out/ab_new_$i.log 2>&1 \
      || { tail -20 gpurun_out/ab_new_$i.log; exit 1; }
    echo "old: $(grep -o '"ms_per_step": [0-9.]*' gpurun_out/ab_old_$i.log)  new: $(grep -o '"ms_per_step": [0-9.]*' gpurun_out/ab_new_$i.log)"
  done ;;
qcurve)
  mkdir -p gpurun_out/qc; : > gpurun_out/qc/qcurve.txt
  for spec in ${SPECS:-"all 1" "all 2" "all 4" "all 5" "all 8" "all 16" "kernels 2" "kernels 5" "kernels 10" "kernels 16"}; do
    set -- $spec
    DTYPE=fp32 RESET=$1 timeout -k 10 200 python -u tools/probe_pop.py $2 $2 1 1 > gpurun_out/qc/run.log 2>&1 \
      || { tail -5 gpurun_out/qc/run.log; exit 1; }
    echo "== RESET=$1 P=$2 $(grep '^{' gpurun_out/qc/run.log | cut -c1-200)" | tee -a gpurun_out/qc/qcurve.txt
  done ;;
ga)
  heartbeat; ck=${CKPT:-gpurun_out/ga/ckpt}; mkdir -p gpurun_out/ga "$(dirname "$ck")"
  if [ -n "${SEED_CKPT:-}" ] && [ -d "$SEED_CKPT" ] && [ ! -d "$ck" ]; then cp -r "$SEED_CKPT" "$ck"; fi
  timeout -k 10 ${TIME:-1080} python3 -u tools/ga_run.py --gens ${GENS:-20} --ckpt "$ck" --resume \
    --time-budget ${BUDGET:-900} ${GA_ARGS:-} > gpurun_out/ga/run${TAG:-}.json 2> gpurun_out/ga/run${TAG:-}.err; rc=$?
  grep "\[ga_run\]" gpurun_out/ga/run${TAG:-}.err | tail -25; cat gpurun_out/ga/run${TAG:-}.json
  exit $rc ;;
gbdt)
  timeout -k 10 300 python -u -m pytest tests/test_gbdt_gpu.py -x -q --timeout 120 --timeout-method thread \
    > gpurun_out/gbdt_tests.log 2>&1 || { tail -30 gpurun_out/gbdt_tests.log; exit 1; }
  tail -1 gpurun_out/gbdt_tests.log
  if [ -n "${BENCH:-}" ]; then
    timeout -k 10 600 python tools/bench_gbdt.py --pop ${POP:-8} --rounds ${ROUNDS:-50} ${GBDT_ARGS:-} > gpurun_out/bench_gbdt.log 2>&1 \
      || { tail -10 gpurun_out/bench_gbdt.log; exit 1; }
    grep "{" gpurun_out/bench_gbdt.log
  fi
  rocprof_env; rm -rf /tmp/pg; mkdir -p gpurun_out/prof_gbdt
  GENTUN_GBDT_TIMING=1 timeout -k 10 300 rocprofv3 --kernel-trace --stats -d /tmp/pg -o run --output-format csv -- \
    python3 tools/probe_gbdt.py 1000000 256 ${DEPTH:-10} 5 > gpurun_out/prof_gbdt/run.log 2>&1 \
    || { tail -5 gpurun_out/prof_gbdt/run.log; exit 1; }
  find /tmp/pg -name "*kernel_stats.csv" -exec cp {} gpurun_out/prof_gbdt/ \;
  grep "{\|gbdt_hip" gpurun_out/prof_gbdt/run.log | tail -2
  head -12 gpurun_out/prof_gbdt/run_kernel_stats.csv | cut -d, -f1-4 ;;
gbdt-predict)
  timeout -k 10 ${TIME:-420} python -u tools/bench_gbdt_predict.py --rows ${ROWS:-1000000} --features ${FEATURES:-256} \
    --trees ${TREES:-500} --depth ${DEPTH:-6} --threads ${THREADS:-16} ${PREDICT_ARGS:-} \
    2>&1 | tail -3 | cut -c1-900          # the result line; the script's status is the bench's (pipefail)
  exit $? ;;
gbdt-shap)
  heartbeat
  timeout -k 10 ${TIME:-560} python -u tools/bench_gbdt_shap.py --rows ${ROWS:-200000} --features ${FEATURES:-256} \
    --trees ${TREES:-500} --depth ${DEPTH:-6} --threads ${THREADS:-16} ${SHAP_ARGS:-} \
    2>&1 | tail -3 | cut -c1-900          # the result line; the script's status is the bench's (pipefail)
  exit $? ;;
gbdt-interactions)
  heartbeat
  timeout -k 10 ${TIME:-300} python -u tools/bench_gbdt_shap.py --interactions --rows ${ROWS:-20000} \
    --features ${FEATURES:-32} --trees ${TREES:-500} --depth ${DEPTH:-6} --threads ${THREADS:-16} \
    --splits ${SPLITS:-0} ${SHAP_ARGS:-} \
    2>&1 | tail -3 | cut -c1-1200         # the result line; the script's status is the bench's (pipefail)
  exit $? ;;
cnn-predict)
  timeout -k 10 ${TIME:-420} python -u tools/bench_cnn_predict.py --rows ${ROWS:-10000} --reps ${REPS:-5} ${PREDICT_ARGS:-} \
    2>&1 | tail -3 | cut -c1-2400         # the result line; the script's status is the bench's (pipefail)
  exit $? ;;
cnn-ensemble)
  timeout -k 10 ${TIME:-540} python -u tools/bench_cnn_ensemble.py --rows ${ROWS:-10000} --reps ${REPS:-5} --k ${K:-4,16} \
    --fit-rows ${FIT_ROWS:-2000} ${ENSEMBLE_ARGS:-} \
    2>&1 | tail -3 | cut -c1-4000         # the result line; the script's status is the bench's (pipefail)
  exit $? ;;
cnn-augment)
  # step time without / with augmentation (and in ab_old/, the built parent tree, when it is there), then the
  # kernel's own time from a kernel trace of one child run of its own; files are kept under $OUT
  out=${OUT:-/tmp/cnn_augment}; heartbeat; mkdir -p $out; rocprof_env; rm -rf /tmp/prof_aug
  parent=""; [ -d ab_old/gentun_amd/_native ] && parent="--parent ab_old"
  timeout -k 10 ${TIME:-700} python -u tools/bench_augment.py --groups ${GROUPS_LIST:-25,80} --reps ${REPS:-3} $parent \
    > $out/bench.json 2> $out/bench.err &&
  cut -c1-3000 $out/bench.json &&
  timeout -k 10 300 rocprofv3 --kernel-trace --stats -d /tmp/prof_aug -o run --output-format csv -- \
    python3 tools/bench_augment.py --child .:${PROF_GROUPS:-25}:1 > $out/prof.log 2>&1 &&
  find /tmp/prof_aug -name "*kernel_stats.csv" -exec cp {} $out/kernel_stats.csv \; &&
  grep -E "Name|augment" $out/kernel_stats.csv | cut -c1-300; rc=$?
  [ $rc -eq 0 ] || tail -5 $out/bench.err $out/prof.log 2>/dev/null
  exit $rc ;;
cnn-distill)
  # step time on hard labels / smoothed labels / a target table (and in ab_old/, the built parent tree, when it is
  # there), then the head kernels' own time from a kernel trace of one child run of its own, then the
  # distillation record; files are kept under $OUT
  out=${OUT:-/tmp/cnn_distill}; heartbeat; mkdir -p $out; rocprof_env; rm -rf /tmp/prof_distill
  parent=""; [ -d ab_old/gentun_amd/_native ] && parent="--parent ab_old"
  timeout -k 10 ${TIME:-900} python -u tools/bench_distill.py --groups ${GROUPS_LIST:-25,80} --reps ${REPS:-5} $parent \
    > $out/bench.json 2> $out/bench.err &&
  cut -c1-4000 $out/bench.json &&
  timeout -k 10 300 rocprofv3 --kernel-trace --stats -d /tmp/prof_distill -o run --output-format csv -- \
    python3 tools/bench_distill.py --child .:${PROF_GROUPS:-25}:table > $out/prof.log 2>&1 &&
  find /tmp/prof_distill -name "*kernel_stats.csv" -exec cp {} $out/kernel_stats.csv \; &&
  grep -E "Name|head_" $out/kernel_stats.csv | cut -c1-300 &&
  { [ "${ACC:-1}" = 0 ] || { timeout -k 10 ${ACC_TIME:-600} python -u tools/bench_distill.py --accuracy \
    > $out/accuracy.json 2> $out/accuracy.err && cut -c1-3000 $out/accuracy.json; }; }; rc=$?
  [ $rc -eq 0 ] || tail -5 $out/bench.err $out/prof.log $out/accuracy.err 2>/dev/null
  exit $rc ;;
cnn-tta)
  # the result line is printed; the files are kept under $OUT
  out=${OUT:-/tmp/cnn_tta}; heartbeat; mkdir -p $out
  timeout -k 10 ${TIME:-420} python -u tools/bench_cnn_tta.py --rows ${ROWS:-10000} --fit-rows ${FIT_ROWS:-2000} \
    --k ${K:-4} --reps ${REPS:-5} ${TTA_ARGS:-} > $out/bench.json 2> $out/bench.err; rc=$?
  [ $rc -eq 0 ] && cut -c1-6000 $out/bench.json || tail -5 $out/bench.err
  exit $rc ;;
cnn-occlusion)
  # one line per finished case, then the result line; the files are kept under $OUT
  out=${OUT:-/tmp/cnn_occlusion}; heartbeat; mkdir -p $out
  timeout -k 10 ${TIME:-900} python -u tools/bench_cnn_occlusion.py --rows ${ROWS:-1000} --fit-rows ${FIT_ROWS:-2000} \
    --k ${K:-4} --reps ${REPS:-5} ${OCC_ARGS:-} > $out/bench.json 2> $out/bench.err; rc=$?
  [ $rc -eq 0 ] && tail -1 $out/bench.json | cut -c1-8000 || { tail -5 $out/bench.err; cut -c1-2000 $out/bench.json; }
  exit $rc ;;
cnn-gradcam)
  # the result line, then the new kernels' own durations from a kernel trace of one child run of its own (fits,
  # then three gradcam calls per model); the files are kept under $OUT
  out=${OUT:-/tmp/cnn_gradcam}; heartbeat; mkdir -p $out; rocprof_env; rm -rf /tmp/prof_cam
  timeout -k 10 ${TIME:-900} python -u tools/bench_cnn_gradcam.py --rows ${ROWS:-10000} --occ-rows ${OCC_ROWS:-1000} \
    --fit-rows ${FIT_ROWS:-2000} --k ${K:-4} --reps ${REPS:-5} ${CAM_ARGS:-} > $out/bench.json 2> $out/bench.err &&
  tail -1 $out/bench.json | cut -c1-8000 &&
  timeout -k 10 300 rocprofv3 --kernel-trace --stats -d /tmp/prof_cam -o run --output-format csv -- \
    python3 tools/bench_cnn_gradcam.py --trace --rows ${ROWS:-10000} --fit-rows ${FIT_ROWS:-2000} --k ${K:-4} \
    ${CAM_ARGS:-} > $out/prof.log 2>&1 &&
  find /tmp/prof_cam -name "*kernel_stats.csv" -exec cp {} $out/kernel_stats.csv \; &&
  grep -E "Name|gradcam|w1sum|head_predict|head_ensemble|dense_fwd" $out/kernel_stats.csv | cut -c1-300; rc=$?
  [ $rc -eq 0 ] || { tail -5 $out/bench.err $out/prof.log 2>/dev/null; cut -c1-2000 $out/bench.json; }
  exit $rc ;;
rehearse)
  heartbeat
  GENTUN_DIST_BACKEND=gloo timeout -k 10 600 python -m torch.distributed.run --nnodes=1 --nproc-per-node ${N:-2} \
    --master-addr 127.0.0.1 --master-port 29533 bench.py --gpus ${N:-2} --steps ${STEPS:-2} --warmup 1 \
    > gpurun_out/rehearse.json 2> gpurun_out/rehearse.err || { tail -20 gpurun_out/rehearse.err; exit 1; }
  cut -c1-600 gpurun_out/rehearse.json ;;
secondary)
  heartbeat; mkdir -p gpurun_out/sec
  if [ -z "${SKIP_KERNELS:-}" ]; then
    timeout -k 10 ${KTIME:-560} python3 -u bench.py --gpus 1 --fold-reset kernels --steps ${KSTEPS:-3} --warmup 1 \
      --json-out gpurun_out/sec/kernels.json > gpurun_out/sec/kernels.out 2> gpurun_out/sec/kernels.err \
      || { tail -5 gpurun_out/sec/kernels.err; exit 1; }
    cat gpurun_out/sec/kernels.json
  fi
  if [ -z "${SKIP_TORCH:-}" ]; then
    timeout -k 10 ${TTIME:-560} python3 -u bench.py --gpus 1 --backend torch --steps ${TSTEPS:-2} --warmup 1 \
      --json-out gpurun_out/sec/torch.json > gpurun_out/sec/torch.out 2> gpurun_out/sec/torch.err \
      || { tail -5 gpurun_out/sec/torch.err; exit 1; }
    cat gpurun_out/sec/torch.json
  fi ;;
*)
  sed -n 2,25p "$0"; exit 2 ;;
esac
