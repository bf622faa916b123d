# A/B of the emitted 256-bit code on a GPU box: bench lines with the emitted code (CW_FP_JIT=1) and with the interpreter
set -x
OUT=${OUT:-bench_lines}; mkdir -p $OUT     # where the bench lines go
for jit in ${JITS:-1}; do
  CW_FP_JIT=$jit python bench.py --full --workload poseidon2 --steps 20 --warmup 3 --no-cpu-baseline > $OUT/ab_poseidon2_jit$jit.json 2> $OUT/ab_poseidon2_jit$jit.err
  CW_FP_JIT=$jit python bench.py --full --workload semaphore20p --total-batch 8192 --shard-of 8 --steps 10 --warmup 2 --no-cpu-baseline > $OUT/ab_sem_shard_jit$jit.json 2> $OUT/ab_sem_shard_jit$jit.err
  CW_FP_JIT=$jit python bench.py --full --workload semaphore20p --steps 10 --warmup 2 --no-cpu-baseline > $OUT/ab_sem8192_jit$jit.json 2> $OUT/ab_sem8192_jit$jit.err
done
tail -c 300 $OUT/*.err
