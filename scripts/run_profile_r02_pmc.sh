# Round-2 PMC passes of the headline step (separate passes, kernel trace only; never TA_*/TCP_* counters: they have hung the
# GPU) + the bench line they are matched with.  Run from the repo root; the summary lands in
# $OUT/r02_pmc.json (default profile_out/; copy to profiles/r02_pmc.json: bench.py attaches it when the kernel-source hash matches).
R=$(pwd); OUT=${OUT:-$R/profile_out}
mkdir -p $OUT
timeout 600 python bench.py --full --no-cpu-baseline > $OUT/bench_for_pmc.json 2>/dev/null
cd /tmp && export TMPDIR=/tmp
CMD="python $R/bench.py --steps 2 --warmup 1 --preheat-seconds 0 --no-graphs --no-kernel-events --no-cpu-baseline"
for pass in "FETCH_SIZE" "WRITE_SIZE" "SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES SQ_INSTS_VALU"; do
  tag=$(echo $pass | cut -d' ' -f1)
  rm -rf /tmp/pmc_final_$tag
  timeout 400 rocprofv3 --kernel-trace --pmc $pass -d /tmp/pmc_final_$tag -o p -- $CMD > /dev/null 2>&1
  echo "$tag rc=$?"
  mkdir -p /tmp/pmcflat/pmc_final_$tag; cp $(find /tmp/pmc_final_$tag -name '*.db' | head -1) /tmp/pmcflat/pmc_final_$tag/p_results.db
done
cd $R
python scripts/pmc_summary.py /tmp/pmcflat $OUT/r02_pmc.json $OUT/bench_for_pmc.json | tail -16
