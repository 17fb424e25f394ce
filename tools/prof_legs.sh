# rocprofv3 kernel stats of bench.py's config 3 / 4 / 5 legs (one run).  Run on the GPU box; summary -> prof_out/<tag>_legs_kernel_stats.md (usage: bash tools/prof_legs.sh [tag=r04])
set -e
R=$GRAFT_REPO_ROOT
OUT=$R/prof_out; mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
timeout -k 10 500 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_legs -o p -- python3 $R/bench.py --full --legs-only --leg config3_vq_argmin,config4_vicreg_step,config5_ntxent_step --repeats 1 --no-cpu-baseline > $OUT/prof_legs.log 2>&1 || (tail -5 $OUT/prof_legs.log; exit 1)
cd $R
python tools/profile_summary.py stats $OUT/prof_legs/p_kernel_stats.csv 1 $OUT/${1:-r04}_legs_kernel_stats.md
head -40 $OUT/${1:-r04}_legs_kernel_stats.md
