# Regenerates the committed profile evidence of a round:  bash scripts/gpu_profile_round.sh r02
# (writes under ${OUT:-results}/<round>/, scripts/copy_profiles.sh copies the summaries into profiles/; every GPU step has its own
# time limit and the first step that fails ends the run)
set -e -o pipefail
R=${1:-r05}; O=${OUT:-results}/$R
mkdir -p $O; export TMPDIR=/tmp; export PYTHONPATH=$PWD
PMC_SQ="SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_INSTS_MFMA SQ_INSTS_VALU SQ_WAVE_CYCLES SQ_WAIT_INST_ANY SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE"
Q="--no-cpu-baseline --no-pca-hard --no-e2e"
# the full line of the default workload (500k x 100k headline, exact-integer mode; carries the fp64 kernels' numbers as
# fp64_mode, the CPU baseline and both PCA solves), then the other workloads and the explicit modes
timeout -k 10 900 python bench.py --full > $O/bench_cfg3_n1.json 2> $O/bench_cfg3_n1.err
timeout -k 10 900 python bench.py --full --workload cfg2 > $O/bench_cfg2_n1.json 2>/dev/null
for a in fp64 fp32 i8x4; do
  timeout -k 10 900 python bench.py --full --workload cfg2 --accum $a $Q --no-alt > $O/bench_cfg2_n1_$a.json 2>/dev/null
  timeout -k 10 900 python bench.py --full --workload cfg3 --accum $a $Q --no-alt > $O/bench_cfg3_n1_$a.json 2>/dev/null
done
for wl in cfg4shard cfg5shard; do timeout -k 10 900 python bench.py --full --workload $wl $Q > $O/bench_${wl}_n1.json 2>/dev/null; done
timeout -k 10 900 python bench.py --full --workload cfg4shard --accum i8x4 $Q --no-alt > $O/bench_cfg4shard_n1_i8x4.json 2>/dev/null   # the cheap passes' kernels on the shard
timeout -k 10 900 python bench.py --full --workload cfg5shard --accum fp32 $Q --no-alt > $O/bench_cfg5shard_n1_fp32.json 2>/dev/null
for a in i8 fp64; do
  # kernel trace of the full line for the default mode (same flags), of --accum fp64 for the other
  if [ $a = i8 ]; then X=""; else X="--accum fp64 $Q --no-alt"; fi
  timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $O/trace_cfg3_$a -o bench -- python bench.py --full $X > /dev/null 2>&1
  timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $O/trace_cfg2_$a -o bench -- python bench.py --full --workload cfg2 --accum $a $Q --no-alt > /dev/null 2>&1
  for wl in cfg2 cfg3; do
    st=3; [ $wl = cfg3 ] && st=2
    for kind in fetch write sq; do
      case $kind in fetch) C="FETCH_SIZE";; write) C="WRITE_SIZE";; sq) C="--kernel-trace $PMC_SQ";; esac
      if [ $kind = sq ]; then
        timeout -k 10 400 rocprofv3 --kernel-trace --pmc $PMC_SQ --output-format csv -d $O/pmc_${kind}_${wl}_$a -o pmc -- python bench.py --workload $wl --accum $a --steps $st --warmup 1 --no-cpu-baseline --no-pca --no-alt --no-e2e --traffic none > /dev/null 2>&1
      else
        timeout -k 10 400 rocprofv3 --pmc $C --output-format csv -d $O/pmc_${kind}_${wl}_$a -o pmc -- python bench.py --workload $wl --accum $a --steps $st --warmup 1 --no-cpu-baseline --no-pca --no-alt --no-e2e --traffic none > /dev/null 2>&1
      fi
    done
  done
done
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $O/trace_cfg4shard_i8 -o bench -- python bench.py --full --workload cfg4shard $Q --no-alt > /dev/null 2>&1
python scripts/summarise_pmc.py $O _fp64 > $O/pmc_summary.json
python scripts/summarise_pmc.py $O _i8 > $O/pmc_summary_i8.json
timeout -k 10 900 python scripts/mfma_i8_peak.py > $O/mfma_i8_microbench.txt 2>&1
timeout -k 10 900 python scripts/mfma_peak.py > $O/mfma_f64_microbench.txt 2>&1
timeout -k 10 900 python bench.py --full --workload cfg5 $Q --no-e2e > $O/bench_cfg5_n1.json 2>/dev/null
timeout -k 10 900 python bench.py --full --blockvec 32 $Q --no-e2e --no-alt > $O/bench_cfg3_n1_b32.json 2>/dev/null
timeout -k 10 900 python scripts/ortho_slice_cost.py > $O/ortho_slice_cost.txt 2>&1
timeout -k 10 900 python scripts/partial_download_probe.py > $O/partial_download.txt 2>&1
timeout -k 10 900 python scripts/solve_profiles.py 2 > $O/solve_profiles.txt 2>&1
timeout -k 10 900 python scripts/k4_bench.py > $O/k4_bench.txt 2>&1
timeout -k 10 900 python scripts/fp_apply_bench.py > $O/fp_apply_bench.txt 2>&1
timeout -k 10 900 python scripts/missing_routes_probe.py > $O/missing_routes.txt 2>&1
FPCA_TIMING=1 timeout -k 10 900 bash scripts/gpu_cli_e2e.sh 500000 100000 3 > $O/cli_e2e_cfg3.txt 2>&1
timeout -k 10 600 bash scripts/power_sample.sh i8 > $O/power_sample.txt 2>&1
for t in trace_cfg3_i8 trace_cfg3_fp64 trace_cfg4shard_i8; do python scripts/summarise_trace.py $O/$t > $O/${t}_by_grid.csv; done
# slim the raw traces before they travel back (the stats CSVs are what profiles/ keeps)
find $O -name "*kernel_trace.csv" -size +2M -delete; find $O -name "*counter_collection.csv" -size +8M -delete
head -70 $O/pmc_summary_i8.json; tail -c 1500 $O/bench_cfg3_n1.json
