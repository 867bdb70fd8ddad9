cd /tmp && export TMPDIR=/tmp
root=${GRAFT_REPO_ROOT}
trace=$(mktemp -d)
timeout 300 rocprofv3 --kernel-trace --output-format csv -d $trace -- python $root/bench.py --full --no-cpu-baseline --no-parity --no-extra --sustained-steps 0 --steps 600 --warmup 100 --burn-in 300 > /dev/null 2>&1
python $root/tools/probes/launch_gaps.py $trace
rm -rf $trace
