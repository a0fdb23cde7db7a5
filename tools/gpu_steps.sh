#!/bin/bash
# One parametrised script for the GPU box (replaces the per-run ab_*.sh / r2_*.sh / r3_*.sh scripts of earlier rounds):
#     gpurun --timeout 900 -- 'bash tools/gpu_steps.sh TAG step [step ...]'
# Every step writes under gpurun_out/TAG and prints one status line; a failed or timed-out GPU step ends the script
# (no further GPU step is started after one that was killed).  Steps:
#   smoke           __graft_entry__.smoke()
#   tests           the whole GPU suite;           tests:EXPR  -> pytest -k EXPR
#   bench           the judged line with everything else it measures (bench.py --full) + a short digest
#   scenes[:names]  tools/bench_scenes.py [names, comma separated]
#   refidx          tools/ref_indexing_diff.py on configs 4 and 5 (GPU)
#   editcost        tools/edit_cost.py: vrt_update_voxels against upload + prepare -> the table of profiles/edit_cost.md, written under this run's output folder
#   castrate[:MAXN] tools/cast_rate.py: Mrays/s of vrt_cast_rays per batch size, both kernel instantiations -> cast_rate.md + the raw lines, under this run's output folder
#   radiancerate    tools/radiance_rate.py: path-samples/s of vrt_trace_radiance next to the fused render kernel's -> radiance_rate.jsonl under this run's output folder
#   sensorrate      tools/sensor_rate.py: items/s of vrt_gather_irradiance next to vrt_trace_radiance on as many items -> sensor_rate.jsonl under this run's output folder
#   proberate       tools/probe_rate.py: probes/s of vrt_gather_probes next to host-drawn directions through vrt_trace_radiance -> probe_rate.jsonl under this run's output folder
#   sweeprate       tools/sweep_rate.py: boxes/s of vrt_sweep_boxes next to vrt_cast_rays on as many rays -> sweep_rate.jsonl under this run's output folder
#   voxelizerate    tools/voxelize_rate.py: ms a call of vrt_voxelize_triangles next to vrt_update_voxels of the same box -> voxelize_rate.jsonl under this run's output folder
#   fillrate        tools/fill_rate.py: ms a call of vrt_fill_triangles next to vrt_voxelize_triangles of the same mesh and vrt_update_voxels of the same box -> fill_rate.jsonl under this run's output folder
#   distancerate    tools/distance_rate.py: ms a call of vrt_distance_field (d2; d2 + nearest) next to vrt_fetch_voxels of the same box -> distance_rate.jsonl under this run's output folder
#   labelrate       tools/label_rate.py: ms a call of vrt_label_components next to vrt_fetch_voxels and vrt_distance_field of the same box -> label_rate.jsonl under this run's output folder
#   moverate        tools/move_rate.py: ms a call of vrt_move_voxels next to vrt_update_voxels of the same box and to fetch + torch.where + update -> move_rate.jsonl under this run's output folder
#   labelkernels    tools/label_kernels.py: the three k_label_* kernels' durations per configuration, from a kernel trace -> label_kernels.jsonl under this run's output folder
#   trace:CASE      rocprofv3 --kernel-trace --stats of bench_scenes.py CASE (CASE = bench: the bench command, config 2)
#   pmc:CASE        tools/pmc.sh CASE + summary
#   timeline:CASE[:MODE[:LAG]]  launches and copies in time (tools/timeline.py)
#   predict:CONFIG[:N,..]  predicted N-GPU step times (tools/predict_scaling.py)
#   traffic         counters of every config -> profiles/traffic.json for this build;  present: present rates;  pmcdefault: the default schedule under --pmc
#   diag:NAME:ARGS       tools/diag_regions.py ARGS (comma separated) with build_variants/libvrt_NAME.so (a -DVRT_DIAG_REGIONS build)
#   variant:NAME:CASES   tools/bench_scenes.py CASES (comma separated) with build_variants/libvrt_NAME.so (built beforehand: tools/build_variant.sh)
set -o pipefail
TAG=$1; shift
O=$GRAFT_REPO_ROOT/gpurun_out/$TAG; mkdir -p $O
cd $GRAFT_REPO_ROOT
fail() { local rc=${2:-1}; [ "$rc" == 0 ] && rc=1; echo "$1 FAILED rc=$rc"; exit $rc; }   # (never 0: a later step must not start)
for step in "$@"; do
  name=${step%%:*}; arg=${step#*:}; [ "$arg" == "$step" ] && arg=""
  case $name in
    smoke)
      timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1 || fail smoke $?
      tail -1 $O/smoke.log ;;
    tests)
      if [ -n "$arg" ]; then timeout -k 10 1000 python -m pytest tests/ -x -q -m gpu -k "$arg" > $O/pytest_gpu.log 2>&1 || { rc=$?; tail -30 $O/pytest_gpu.log; fail tests $rc; }
      else timeout -k 10 1000 python -m pytest tests/ -x -q -m gpu > $O/pytest_gpu.log 2>&1 || { rc=$?; tail -30 $O/pytest_gpu.log; fail tests $rc; }; fi
      tail -1 $O/pytest_gpu.log ;;
    bench)
      timeout -k 10 600 python bench.py --full $arg > $O/bench.json 2> $O/bench.err || { rc=$?; tail -5 $O/bench.err; fail bench $rc; }
      python tools/bench_digest.py $O/bench.json ;;
    scenes)
      timeout -k 10 900 python tools/bench_scenes.py ${arg//,/ } > $O/scenes${arg:+_}${arg//,/_}.jsonl 2> $O/scenes.err || { rc=$?; tail -5 $O/scenes.err; fail scenes $rc; }
      python -c "
import json,sys
for l in open('$O/scenes${arg:+_}${arg//,/_}.jsonl'):
    d=json.loads(l); print(' ', d.get('name'), d.get('mpaths_per_s'), {k:v for k,v in d.items() if k.endswith('_ms')})" ;;
    refidx)
      for c in 4 5; do timeout -k 10 600 python tools/ref_indexing_diff.py --backend gpu --config $c > $O/refidx_config$c.json 2> $O/refidx.err || { rc=$?; tail -5 $O/refidx.err; fail refidx $rc; }; cat $O/refidx_config$c.json; done ;;
    editcost)
      timeout -k 10 300 python tools/edit_cost.py --out $O/edit_cost.md > $O/edit_cost.jsonl 2> $O/edit_cost.err || { rc=$?; tail -5 $O/edit_cost.err; fail editcost $rc; }
      cat $O/edit_cost.md ;;
    castrate)
      timeout -k 10 500 python tools/cast_rate.py ${arg:+--max-n $arg} --out $O/cast_rate.md > $O/cast_rate.jsonl 2> $O/cast_rate.err || { rc=$?; tail -5 $O/cast_rate.err; fail castrate $rc; }
      tail -1 $O/cast_rate.jsonl ;;
    radiancerate)
      timeout -k 10 300 python tools/radiance_rate.py --out $O/radiance_rate.jsonl > $O/radiance_rate.out 2> $O/radiance_rate.err || { rc=$?; tail -5 $O/radiance_rate.err; fail radiancerate $rc; }
      tail -1 $O/radiance_rate.out ;;
    sensorrate)
      timeout -k 10 300 python tools/sensor_rate.py --out $O/sensor_rate.jsonl > $O/sensor_rate.out 2> $O/sensor_rate.err || { rc=$?; tail -5 $O/sensor_rate.err; fail sensorrate $rc; }
      tail -1 $O/sensor_rate.out ;;
    proberate)
      timeout -k 10 300 python tools/probe_rate.py --out $O/probe_rate.jsonl > $O/probe_rate.out 2> $O/probe_rate.err || { rc=$?; tail -5 $O/probe_rate.err; fail proberate $rc; }
      tail -1 $O/probe_rate.out ;;
    sweeprate)
      timeout -k 10 300 python tools/sweep_rate.py --out $O/sweep_rate.jsonl > $O/sweep_rate.out 2> $O/sweep_rate.err || { rc=$?; tail -5 $O/sweep_rate.err; fail sweeprate $rc; }
      tail -1 $O/sweep_rate.out ;;
    voxelizerate)
      timeout -k 10 300 python tools/voxelize_rate.py --out $O/voxelize_rate.jsonl > $O/voxelize_rate.out 2> $O/voxelize_rate.err || { rc=$?; tail -5 $O/voxelize_rate.err; fail voxelizerate $rc; }
      tail -1 $O/voxelize_rate.out ;;
    fillrate)
      timeout -k 10 300 python tools/fill_rate.py --out $O/fill_rate.jsonl > $O/fill_rate.out 2> $O/fill_rate.err || { rc=$?; tail -5 $O/fill_rate.err; fail fillrate $rc; }
      tail -1 $O/fill_rate.out ;;
    distancerate)
      timeout -k 10 300 python tools/distance_rate.py --out $O/distance_rate.jsonl > $O/distance_rate.out 2> $O/distance_rate.err || { rc=$?; tail -5 $O/distance_rate.err; fail distancerate $rc; }
      tail -1 $O/distance_rate.out ;;
    labelrate)
      timeout -k 10 300 python tools/label_rate.py --out $O/label_rate.jsonl > $O/label_rate.out 2> $O/label_rate.err || { rc=$?; tail -5 $O/label_rate.err; fail labelrate $rc; }
      tail -2 $O/label_rate.out ;;
    moverate)
      timeout -k 10 420 python tools/move_rate.py --out $O/move_rate.jsonl > $O/move_rate.out 2> $O/move_rate.err || { rc=$?; tail -5 $O/move_rate.err; fail moverate $rc; }
      tail -2 $O/move_rate.out ;;
    labelkernels)
      here=$PWD   # (the repository's root: the script has changed into it)
      ( cd /tmp; export TMPDIR=/tmp; timeout -k 10 240 rocprofv3 --kernel-trace --output-format csv -d $O/trace_label -o t -- python $here/tools/label_kernels.py run > $O/label_kernels.out 2> $O/label_kernels.err ) || fail labelkernels $?
      python tools/label_kernels.py digest $O/trace_label $O/label_kernels.jsonl; rm -rf $O/trace_label ;;
    trace)
      ( cd /tmp; export TMPDIR=/tmp
        if [ "$arg" == "bench" ]; then timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/trace_bench -o t -- python $GRAFT_REPO_ROOT/bench.py --no-cpu-baseline --no-secondary > $O/bench_under_rocprof.json 2> $O/trace_bench.err
        else timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/trace_$arg -o t -- python $GRAFT_REPO_ROOT/tools/bench_scenes.py $arg > $O/trace_$arg.jsonl 2> $O/trace_$arg.err; fi ) || fail trace:$arg $?
      f=$(find $O/trace_$arg -name '*kernel_stats.csv' | head -1); [ -n "$f" ] && cp $f $O/${arg}_kernel_stats.csv && head -8 $O/${arg}_kernel_stats.csv | cut -c1-160
      find $O -name '*kernel_trace.csv' -delete; find $O -name '*.db' -delete ;;
    pmc)
      bash tools/pmc.sh $arg ${TAG}_pmc_$arg > /dev/null 2>&1 || fail pmc:$arg $?
      python tools/pmc_summary.py $GRAFT_REPO_ROOT/gpurun_out/${TAG}_pmc_$arg > $O/pmc_$arg.txt; rm -rf gpurun_out/${TAG}_pmc_$arg
      echo "pmc $arg: $(grep -c mean $O/pmc_$arg.txt) rows" ;;
    variant)
      IFS=: read -r vname vcases <<< "$arg"
      VRT_LIB_PATH=$GRAFT_REPO_ROOT/build_variants/libvrt_$vname.so timeout -k 10 600 python tools/bench_scenes.py ${vcases//,/ } > $O/variant_$vname.jsonl 2> $O/variant_$vname.err || { rc=$?; tail -5 $O/variant_$vname.err; fail variant:$vname $rc; }
      python -c "
import json
for l in open('$O/variant_$vname.jsonl'):
    d=json.loads(l); print('  [$vname]', d.get('name'), d.get('mpaths_per_s'), {k:v for k,v in d.items() if k.endswith('_ms')})" ;;
    traffic)   # counters per config (tools/pmc.sh) -> profiles/traffic.json stamped with the build id; comes back as gpurun_out/TAG/traffic.json
      python -c "from voxel_rt2_amd import _lib; print(_lib.build_id())" > $O/build_id.txt 2>/dev/null
      ID=$(cat $O/build_id.txt); echo "build $ID"
      for c in config2_s1 config5_dense256 config4_dense config3_s6; do
        bash tools/pmc.sh $c ${TAG}_pmc_$c > /dev/null 2>&1 || fail traffic:$c $?
        python tools/pmc_summary.py $GRAFT_REPO_ROOT/gpurun_out/${TAG}_pmc_$c > $O/pmc_$c.txt
        echo "pmc $c: $(grep -c mean $O/pmc_$c.txt) rows"
      done
      python tools/make_traffic.py $ID "$TAG" config2_s1_1080p=gpurun_out/${TAG}_pmc_config2_s1 config5_dense256_4k=gpurun_out/${TAG}_pmc_config5_dense256 \
          config4_dense_4k=gpurun_out/${TAG}_pmc_config4_dense config3_s6_sky_clouds_restir_1080p=gpurun_out/${TAG}_pmc_config3_s6 > $O/traffic_digest.json || fail traffic 1
      cp profiles/traffic.json $O/traffic.json
      rm -rf gpurun_out/${TAG}_pmc_* ;;
    present)   # the frame copied to the host after every step: blocking, asynchronous f32, asynchronous 8 bit
      for mode in 1 async async8; do for lag in 1 2 3; do
        [ $mode == 1 ] && [ $lag != 1 ] && continue
        [ $mode == async ] && [ $lag == 3 ] && continue
        VRT_BENCH_STEPS=120 VRT_BENCH_FETCH_EACH=$mode VRT_BENCH_FETCH_LAG=$lag timeout -k 10 300 python tools/bench_scenes.py config2_s1 config4_dense 2>/dev/null | sed "s/_d8\"/_d8_present_${mode}_lag${lag}\"/; s/_1gpu\"/_1gpu_present_${mode}_lag${lag}\"/" >> $O/present.jsonl
      done; done; echo "present: $(grep -c name $O/present.jsonl)" ;;
    timeline)   # timeline:CASE[:MODE[:LAG]] -> kernel + copy trace of tools/bench_scenes.py CASE (MODE: VRT_BENCH_FETCH_EACH), digested by tools/timeline.py
      IFS=: read -r tcase tmode tlag <<< "$arg"
      ( cd /tmp; export TMPDIR=/tmp VRT_BENCH_STEPS=60 VRT_BENCH_FETCH_EACH=$tmode VRT_BENCH_FETCH_LAG=${tlag:-1}
        timeout -k 10 300 rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -d $O/tl_$tcase$tmode -o t -- python $GRAFT_REPO_ROOT/tools/bench_scenes.py $tcase > $O/tl_$tcase$tmode.jsonl 2> $O/tl_$tcase$tmode.err ) || fail timeline:$arg $?
      python tools/timeline.py $O/tl_$tcase$tmode > $O/timeline_$tcase${tmode:+_}$tmode${tlag:+_lag}$tlag.txt; rm -rf $O/tl_$tcase$tmode
      head -12 $O/timeline_$tcase${tmode:+_}$tmode${tlag:+_lag}$tlag.txt ;;
    predict)   # predict:CONFIG[:N,N,...] -> tools/predict_scaling.py (bench.py --gpus N replayed rank by rank on this GPU)
      IFS=: read -r pcfg pn <<< "$arg"
      timeout -k 10 600 python tools/predict_scaling.py $pcfg ${pn//,/ } > $O/predict_$pcfg.jsonl 2> $O/predict_$pcfg.err || { rc=$?; tail -5 $O/predict_$pcfg.err; fail predict:$arg $rc; }
      python -c "
import json
for l in open('$O/predict_$pcfg.jsonl'):
    d=json.loads(l)
    if 'n_gpus' in d: print('  $pcfg N =', d['n_gpus'], 'equal', d['equal_speedup'], 'balanced', d['balanced_speedup'], {k: v['speedup'] for k, v in d.items() if k.startswith('stripes')})" ;;
    pmcdefault)
      ( cd /tmp; export TMPDIR=/tmp; timeout -k 10 120 rocprofv3 --kernel-trace --pmc SQ_WAVES SQ_INSTS_VALU --output-format csv -d $O/pmc_default -o p -- python $GRAFT_REPO_ROOT/tools/probe_overlap.py > $O/pmc_default_schedule.txt 2>&1 ) || fail pmcdefault $?
      rm -rf $O/pmc_default; tail -2 $O/pmc_default_schedule.txt ;;
    diag)   # diag:NAME:ARGS -> tools/diag_regions.py ARGS with build_variants/libvrt_NAME.so (a -DVRT_DIAG_REGIONS build)
      IFS=: read -r vname dargs <<< "$arg"
      VRT_LIB_PATH=$GRAFT_REPO_ROOT/build_variants/libvrt_$vname.so timeout -k 10 600 python tools/diag_regions.py ${dargs//,/ } > $O/diag_$vname.txt 2> $O/diag_$vname.err || { rc=$?; tail -5 $O/diag_$vname.err; fail diag:$vname $rc; }
      cat $O/diag_$vname.txt ;;
    *) echo "unknown step $step"; exit 64 ;;
  esac
done
