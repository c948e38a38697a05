#!/bin/bash
# Re-takes the committed profiles of the default bench after an edit of csrc/ (tests/test_bench_artefacts.py
# pins them to the hash of the sources): kernel times, counters, the 8-GPU workloads' shares, the headline
# kernel's path counts and instruction mix, and the bench lines.  From the repository root, on an MI355X:
#
#     bash experiments/retake_profiles.sh counters [tag]    # kernel trace, --pmc passes, shares, path counts
#     bash experiments/retake_profiles.sh bench [tag]       # the bench lines (they read the counters just taken)
#
# Both stages write under profiles/ in place (the names bench.py reads) and leave a copy, with the logs, under
# $NDT2D_PROFILE_OUT/prof_<tag>/ (default: profile_out/ in the repository).  Counter passes (rocprofv3 --pmc)
# run on their own; kernel times come from a separate --kernel-trace --stats run.  Before `counters`, on the
# build machine:
#     the library itself (python -m ndt_2d_amd.build), and the path-counter variant experiments/bin/lane_paths.so
#     (ndt2d_match_lane.hip compiled with -DNDT2D_LANE_PATHS, linked with the library's other objects);
#     python3 experiments/asm_loop_mix.py > profiles/r06_valu_mix.json   (static: needs the compiler, no GPU)
# Every step runs under its own time limit and the script stops at the first one that fails.
set -o pipefail
STAGE=${1:?counters|bench}
TAG=${2:-r06}
R=$(cd "$(dirname "$0")/.." && pwd)
O=${NDT2D_PROFILE_OUT:-$R/profile_out}/prof_$TAG
P=$R/profiles
mkdir -p "$O"
export TMPDIR=/tmp
cd /tmp || exit 1

step() {   # step <seconds> <log> <command...>
  local limit=$1 log=$2; shift 2
  timeout -k 10 "$limit" "$@" > "$log" 2>&1
  local rc=$?
  if [ $rc -ne 0 ]; then echo "retake_profiles: '$*' failed with $rc, see $log"; tail -5 "$log"; exit $rc; fi
}

if [ "$STAGE" = counters ]; then
  SIDE="--no-cpu-baseline --no-default-search --no-anchors --no-c-host"
  BENCH="python3 $R/bench.py --full --steps 4 --warmup 2 --prewarm 0 $SIDE"
  step 300 "$O/kt.log" rocprofv3 --kernel-trace --stats --output-format csv -d "$O/kt" -- \
    python3 "$R/bench.py" --full --steps 200 --warmup 10 $SIDE
  find "$O/kt" -name "*kernel_stats.csv" | head -1 | xargs -I{} cp {} "$O/kernel_stats.csv"
  pass() {
    local name=$1; shift
    step 300 "$O/$name.log" rocprofv3 --kernel-trace --pmc "$@" --output-format csv -d "$O/$name" -- $BENCH
  }
  pass sq1 SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CU_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAIT_ANY GRBM_GUI_ACTIVE
  pass sq2 SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_ANY SQ_THREAD_CYCLES_VALU SQ_WAIT_INST_ANY SQ_INSTS_SMEM SQ_INSTS_VMEM SQ_ACTIVE_INST_LDS SQ_ACTIVE_INST_SCA
  pass sq3 SQ_INSTS_VALU_ADD_F64 SQ_INSTS_VALU_MUL_F64 SQ_INSTS_VALU_FMA_F64 SQ_INSTS_VALU_TRANS_F64 SQ_INSTS_VALU_INT32 SQ_INSTS_VALU_INT64 SQ_INSTS_VALU_CVT SQ_INSTS_VALU_FMA_F32
  pass sq4 SQ_INSTS_VALU_ADD_F32 SQ_INSTS_VALU_MUL_F32 SQ_INSTS_VALU_TRANS_F32 SQ_INSTS_FLAT SQ_INSTS_GDS SQ_INSTS_EXP_GDS SQ_INSTS_BRANCH SQ_INSTS_SENDMSG
  pass fetch FETCH_SIZE
  pass write WRITE_SIZE
  python3 "$R/experiments/pmc_to_json.py" "$O" > "$O/pmc_summary.txt" 2> "$O/pmc_to_json.err" || exit 1
  # the 8-GPU workloads share by share on this one GPU
  mkdir -p "$O/shares"
  spass() {
    local name=$1; shift
    step 420 "$O/shares_$name.log" rocprofv3 --kernel-trace --pmc "$@" --output-format csv -d "$O/shares/$name" -- \
      python3 "$R/bench.py" --profile-shares
  }
  spass sq1 SQ_INSTS_VALU SQ_BUSY_CU_CYCLES SQ_WAVES SQ_WAVE_CYCLES SQ_INSTS_SALU SQ_INSTS_LDS SQ_BUSY_CYCLES SQ_WAIT_ANY
  spass sq2 SQ_ACTIVE_INST_VALU SQ_THREAD_CYCLES_VALU SQ_INSTS_VALU_ADD_F64 SQ_INSTS_VALU_MUL_F64 SQ_INSTS_VALU_FMA_F64 SQ_INSTS_VALU_TRANS_F64 SQ_INSTS_VALU_FMA_F32 SQ_INSTS_VALU_ADD_F32
  spass sq3 SQ_INSTS_VALU_MUL_F32 SQ_INSTS_SMEM SQ_INSTS_VMEM SQ_INSTS_VALU_INT32 SQ_INSTS_VALU_INT64 SQ_INSTS_VALU_CVT SQ_INSTS_VALU_TRANS_F32
  spass fetch FETCH_SIZE
  spass write WRITE_SIZE
  python3 "$R/experiments/pmc_shares.py" "$O" "$(python3 "$R/bench.py" --print-source-hash)" > "$O/shares_summary.txt" 2>> "$O/pmc_to_json.err" || exit 1
  cp "$O/pmc.json" "$P/r06_pmc.json"
  cp "$O/kernel_stats.csv" "$P/r06_kernel_stats.csv"
  cp "$O/pmc_summary.txt" "$P/r06_pmc_summary.txt"
  cp "$O/shares_summary.txt" "$P/r06_shares_summary.txt"
  # the headline kernel's dynamic mix: path counts of the -DNDT2D_LANE_PATHS build x the paths' instruction lists,
  # checked class by class against the counters just taken
  NDT2D_HIP_LIB=$R/experiments/bin/lane_paths.so timeout -k 10 120 python3 "$R/experiments/lane_paths.py" 2 \
    > "$P/r06_lane_paths.json" 2> "$O/lane_paths.err" || { echo "lane_paths failed"; tail -5 "$O/lane_paths.err"; exit 1; }
  python3 "$R/experiments/lane_path_mix.py" "$P/r06_lane_paths.json" "$P/r06_pmc.json" > "$P/r06_lane_path_mix.json" \
    2> "$O/lane_path_mix.err" || exit 1
  cp "$P/r06_lane_paths.json" "$P/r06_lane_path_mix.json" "$O/"
  # (the raw traces stay on the machine that took them)
  find "$O" -name "*.csv" -size +1M -delete
  find "$O" -name "*.db" -delete
  cut -c1-150 "$O/kernel_stats.csv" | head -6
  grep -A3 '"remainder"' "$P/r06_lane_path_mix.json" | head -5
elif [ "$STAGE" = bench ]; then
  # stdout = the short line the driver parses, --detail-file = the full record
  timeout -k 10 900 python3 "$R/bench.py" --full --detail-file "$O/bench_detail.json" > "$O/bench.json" 2> "$O/bench.err" \
    || { echo "bench failed"; tail -5 "$O/bench.err"; exit 1; }
  timeout -k 10 900 python3 "$R/bench.py" --full --steps 20 --warmup 5 --detail-file "$O/bench_driver_flags_detail.json" \
    > "$O/bench_driver_flags.json" 2>> "$O/bench.err" || { echo "bench (driver flags) failed"; tail -5 "$O/bench.err"; exit 1; }
  cp "$O/bench.json" "$P/r06_bench.json"
  cp "$O/bench_detail.json" "$P/r06_bench_detail.json"
  cp "$O/bench_driver_flags.json" "$P/r06_bench_driver_flags.json"
  cp "$O/bench_driver_flags_detail.json" "$P/r06_bench_driver_flags_detail.json"
  wc -c "$O/bench.json" "$O/bench_driver_flags.json"
else
  echo "usage: retake_profiles.sh counters|bench [tag]"; exit 2
fi
