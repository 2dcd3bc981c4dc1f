set -o pipefail
mkdir -p gpurun_out/r02h
python -m pytest tests -m gpu -x -q > gpurun_out/r02h/pytest_gpu.log 2>&1; echo "pytest exit $?" >> gpurun_out/r02h/pytest_gpu.log; tail -3 gpurun_out/r02h/pytest_gpu.log
python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > gpurun_out/r02h/smoke.log 2>&1; tail -1 gpurun_out/r02h/smoke.log
bash tools/profile_round.sh r02h > gpurun_out/r02h/profile_round.log 2>&1
python3 bench.py --full --no-cpu-baseline --dtype f32 --eb 1e-4 2>&1 | tail -1
python3 bench.py --full --no-cpu-baseline --mode qt 2>&1 | tail -1
python3 bench.py --full --no-cpu-baseline --dtype f32 --mode qt --eb 1e-4 2>&1 | tail -1
python3 bench.py --full --no-cpu-baseline --no-speculation 2>&1 | tail -1
cat gpurun_out/r02h/bench.json
