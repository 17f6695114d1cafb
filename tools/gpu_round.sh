# one GPU round: GPU tests, bench line, rocprofv3 kernel stats + the two PMC traffic passes of the same command, stress line. Usage: bash tools/gpu_round.sh TAG
set -e
T=${1:-r02}
O=${OUT:-runs}/$T; mkdir -p $O; O=$(cd $O && pwd)
python -m pytest tests -m gpu -x -q > $O/pytest_gpu.log 2>&1 || { tail -30 $O/pytest_gpu.log; exit 1; }
tail -2 $O/pytest_gpu.log
python bench.py --full > $O/bench.json 2> $O/bench.err
python bench.py --stress --full --steps 5 --warmup 2 > $O/bench_stress.json 2> $O/bench_stress.err
R=$PWD
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof -- python3 $R/bench.py --steps 3 --warmup 1 --no-cpu-baseline --ragged-windows 0 --converging-windows 0 --td-windows 0 --no-latency --no-pcie --no-stress-leg > $O/prof_bench.json 2> $O/prof.err
rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $O/pmc_fetch -- python3 $R/bench.py --distinct-lidar 4 --steps 2 --warmup 1 --no-cpu-baseline --ragged-windows 0 --converging-windows 0 --td-windows 0 --no-latency --no-pcie --no-stress-leg > $O/pmc_fetch.json 2> $O/pmc_fetch.err
rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $O/pmc_write -- python3 $R/bench.py --distinct-lidar 4 --steps 2 --warmup 1 --no-cpu-baseline --ragged-windows 0 --converging-windows 0 --td-windows 0 --no-latency --no-pcie --no-stress-leg > $O/pmc_write.json 2> $O/pmc_write.err
find $O -name '*kernel_stats.csv' -o -name '*counter_collection.csv' | head
cd /tmp
rocprofv3 --kernel-trace --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU_MFMA_F64 SQ_INSTS_VALU SQ_WAVE_CYCLES GRBM_GUI_ACTIVE --output-format csv -d $O/pmc_mfma -- python3 $R/bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-lidar-stage --no-marginalize --ragged-windows 0 --converging-windows 0 --td-windows 0 --no-latency --no-pcie --no-stress-leg > $O/pmc_mfma.json 2> $O/pmc_mfma.err
find $O/pmc_mfma -name '*counter_collection.csv' | head -2
cd /tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_stress -- python3 $R/bench.py --stress --stress-windows 32 --steps 3 --warmup 1 --no-cpu-baseline > $O/prof_stress.json 2> $O/prof_stress.err
cd $R
bash tools/dev_batch_sweep.sh $T > $O/batch_sweep.log 2>&1 || true
