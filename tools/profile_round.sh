#!/bin/bash
# Kernel trace + separate PMC passes for the bench workload (run on the GPU box).
#   tools/profile_round.sh <tag>     -> $MHE_OUT/ (default results/): prof_<tag>_{trace,fetch,write,sq}/
set -e
TAG=${1:-r01}
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
export MHE_OUT=${MHE_OUT:-results}; O=$MHE_OUT; mkdir -p "$O"
B="python bench.py --steps 10 --warmup 2 --no-cpu"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_${TAG}_trace -o run -- $B > $O/prof_${TAG}_trace.log 2>&1
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/prof_${TAG}_fetch -o run -- $B > $O/prof_${TAG}_fetch.log 2>&1
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $O/prof_${TAG}_write -o run -- $B > $O/prof_${TAG}_write.log 2>&1
timeout -k 10 300 rocprofv3 --pmc SQ_INSTS_VALU_MFMA_MOPS_F64 SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_WAVE_CYCLES --output-format csv -d $O/prof_${TAG}_sq -o run -- $B > $O/prof_${TAG}_sq.log 2>&1
python tools/parse_pmc.py "$TAG"
# the summary and stats also go next to the other outputs, where tools/collect_records.sh looks
cp profiles/pmc_summary.json "$O/pmc_summary_${TAG}.json"
cp "profiles/${TAG}_kernel_stats.csv" "$O/${TAG}_kernel_stats.csv"
