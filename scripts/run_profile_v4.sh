# Round-1 final tree: default bench line, rocprofv3 kernel-trace summary, PMC passes (separate, kernel-trace only; never
# TA_*/TCP_* counters: they have hung the GPU).  Run from the repo root; results land in $OUT (default profile_out/).
R=$(pwd); OUT=${OUT:-$R/profile_out}
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
CMD="python $R/bench.py --steps 2 --warmup 1 --preheat-seconds 0 --no-graphs --no-kernel-events --no-cpu-baseline"
for pass in "FETCH_SIZE" "WRITE_SIZE" "SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES SQ_INSTS_VALU"; do
  tag=$(echo $pass | cut -d' ' -f1)
  rm -rf $OUT/pmc_final_$tag
  timeout 400 rocprofv3 --kernel-trace --pmc $pass -d $OUT/pmc_final_$tag -o p -- $CMD > /dev/null 2>&1
  echo "$tag rc=$?"
done
python $R/scripts/pmc_summary.py $OUT $OUT/r01_pmc_final.json | tail -5
cp $OUT/r01_pmc_final.json $R/profiles/r01_pmc_final.json      # bench.py reads the traffic figures from here
rm -rf $OUT/prof_v4
timeout 600 rocprofv3 --kernel-trace -d $OUT/prof_v4 -o bench -- python $R/bench.py --full --steps 10 --warmup 3 --no-cpu-baseline > $OUT/bench_under_rocprof.json 2>/dev/null
python $R/scripts/rocpd_stats.py $OUT/prof_v4/bench_results.db > $OUT/r01_bench_n1_kernel_stats_v4.txt 2>&1
rm -rf $OUT/prof_v4 $OUT/pmc_final_*/*.db 2>/dev/null
cd $R
timeout 900 python bench.py --full > $OUT/bench_default.json 2> $OUT/bench_default.err
tail -c 400 $OUT/bench_default.json
