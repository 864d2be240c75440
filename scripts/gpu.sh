#!/bin/bash
# The GPU jobs of this repo, by name (run on the box: gpurun -- 'bash scripts/gpu.sh JOB [ARGS]').
# Every GPU step runs under its own time limit and the first failure ends the job.
#
#   suite                 full GPU test suite + smoke() + the bench line with its sub-results (bench.py --full)
#   tests  PYTEST_ARGS    selected GPU tests (e.g. tests/test_loopback.py)
#   bench  [N] [ARGS]     N runs of `bench.py --steps 200 --warmup 10 --no-extras ARGS`, ms per run
#   line   [ARGS]         one bench line with its sub-results (bench.py --full ARGS) -> bench.json in the output folder
#   prof   MODEL [ARGS]   rocprofv3 kernel trace + per-dispatch breakdown of MODEL's step
#   pmc    COUNTERS CMD   one rocprofv3 --pmc pass (<= the per-block counter limits) over CMD
#   ab     VAR A B [ARGS] alternating bench runs under two values of an environment variable
#   sweep  VAR "V1 V2 .." [ARGS]  bench runs under each value in turn, ROUNDS passes
#   trees  ALT [ARGS]     alternating bench runs of another built source tree ALT against this one
#   tables "T1 T2[@VAR=V]" [ARGS]  alternating bench runs under GEMM tuning tables (DLS_GEMM_TUNING)
#   retune MODEL          exhaustive in-DAG GEMM refinement (benchmarks/refine_dag.py), then an A/B
#                         of the original table against the refined one
#   stamps                in-kernel phase stamps of the GPT-2 GEMM shapes (gpubin/gemm_stamps,
#                         built from benchmarks/gemm_stamps.hip)
#   prefill [ARGS]        chunked prefill: time to the first token with chunk steps against token steps only,
#                         and the chunk attention table (benchmarks/bench_prefill.py ARGS)
#   moe-decode [ARGS]     the skinny grouped expert GEMM against ops.gemm_grouped at Mixtral's shapes, and the
#                         mixtral-8x7b-1l decode step with the skinny launches off and on
#                         (benchmarks/bench_moe_decode.py ARGS)
#   skinny [ARGS]        the dense skinny GEMM against ops.linear / ops.linear_norm at the Llama-3-8B and GPT-2
#                         decode shapes (benchmarks/bench_skinny.py ARGS), then the llama3-8b-1l and gpt2 decode
#                         steps with and without the plan option (benchmarks/decode_step.py --skinny-gemm)
# Output lands in gpurun_out/${TAG:-job}/.
set -o pipefail
ROOT="${GRAFT_REPO_ROOT:-$(pwd)}"
cd "$ROOT"
O="gpurun_out/${TAG:-job}"
mkdir -p "$O"
export DLS_SKIP_BUILD=1
job="$1"; shift

ms() { python -c "import json,sys;print(json.load(open(sys.argv[1]))['ms_per_step'])" "$1"; }

case "$job" in
  suite)
    timeout -k 10 1200 python -u -m pytest tests -x -q -m gpu --timeout 240 --timeout-method thread > $O/pytest_gpu.log 2>&1; rc=$?
    tail -5 $O/pytest_gpu.log; [ $rc -eq 0 ] || exit $rc
    timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1 || { tail -20 $O/smoke.log; exit 3; }
    tail -1 $O/smoke.log
    timeout -k 10 400 python bench.py --full > $O/bench.json 2> $O/bench.err || { tail -20 $O/bench.err; exit 4; }
    cut -c1-600 $O/bench.json
    ;;
  tests)
    timeout -k 10 1100 python -u -m pytest -x -v --timeout 240 --timeout-method thread "$@" > $O/pytest.log 2>&1; rc=$?
    grep -E "PASS|FAIL|ERROR|SKIP" $O/pytest.log | tail -60; tail -3 $O/pytest.log; exit $rc
    ;;
  bench)
    n="${1:-3}"; shift
    for i in $(seq "$n"); do
      timeout -k 10 300 python bench.py --steps 200 --warmup 10 --no-extras "$@" > $O/b$i.json 2> $O/b$i.err || { tail -20 $O/b$i.err; exit 4; }
      echo "run $i: $(ms $O/b$i.json) ms"
    done
    ;;
  line)
    timeout -k 10 600 python bench.py --full "$@" > $O/bench.json 2> $O/bench.err || { tail -20 $O/bench.err; exit 4; }
    cut -c1-3000 $O/bench.json
    ;;
  prof)
    m="$1"; shift
    cd /tmp && export TMPDIR=/tmp
    timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$ROOT/$O/prof_$m" -o k -- \
      python3 "$ROOT/bench.py" --model "$m" --steps 10 --warmup 3 --no-extras "$@" > "$ROOT/$O/prof_$m.log" 2>&1 \
      || { tail -20 "$ROOT/$O/prof_$m.log"; exit 7; }
    python3 "$ROOT/tools/analyze_trace.py" "$ROOT/$O/prof_$m/k_kernel_trace.csv" --steps 5 --per-dispatch > "$ROOT/$O/breakdown_$m.txt" 2>&1
    head -60 "$ROOT/$O/breakdown_$m.txt"
    ;;
  pmc)
    ctr="$1"; shift
    cd /tmp && export TMPDIR=/tmp
    timeout -s KILL 120 rocprofv3 --pmc $ctr --output-format csv -d "$ROOT/$O/pmc" -o p -- "$@" > "$ROOT/$O/pmc.log" 2>&1 \
      || { tail -20 "$ROOT/$O/pmc.log"; exit 8; }
    ls "$ROOT/$O/pmc"
    ;;
  ab)
    var="$1"; a="$2"; b="$3"; shift 3
    for i in $(seq ${ROUNDS:-3}); do
      for v in "$a" "$b"; do
        env "$var=$v" timeout -k 10 300 python bench.py --steps 200 --warmup 10 --no-extras "$@" > $O/ab.json 2> $O/ab.err || { tail -5 $O/ab.err; exit 3; }
        echo "$var=$v $(ms $O/ab.json)"
      done
    done
    ;;
  sweep)
    var="$1"; vals="$2"; shift 2
    for i in $(seq ${ROUNDS:-2}); do
      for v in $vals; do
        env "$var=$v" timeout -k 10 300 python bench.py --steps 200 --warmup 10 --no-extras "$@" > $O/sw.json 2> $O/sw.err || { tail -5 $O/sw.err; exit 3; }
        echo "$var=$v $(ms $O/sw.json)" | tee -a $O/sweep.txt > /dev/null
        echo "$var=$v $(ms $O/sw.json)"
      done
    done
    ;;
  trees)
    alt="$1"; shift
    for i in $(seq ${ROUNDS:-3}); do
      for t in "$alt" .; do
        timeout -k 10 300 python "$t/bench.py" --steps 200 --warmup 10 --no-extras "$@" > $O/t.json 2> $O/t.err || { tail -5 $O/t.err; exit 3; }
        echo "$t $(ms $O/t.json)"
      done
    done
    ;;
  tables)
    tabs="$1"; shift
    for i in $(seq ${ROUNDS:-3}); do
      for e in $tabs; do
        t=${e%%@*}; ev=""; [ "$e" != "$t" ] && ev=${e#*@}; ev=${ev//,/ }
        env DLS_GEMM_TUNING="$t" $ev timeout -k 10 300 python bench.py --no-extras --steps ${STEPS:-200} --warmup 10 "$@" \
          > $O/t.json 2> $O/t.err || { tail -5 $O/t.err; exit 3; }
        echo "$(basename $t) $ev $(ms $O/t.json)" | tee -a $O/tables.txt
      done
    done
    ;;
  retune)
    m="${1:-gpt2}"
    cp distributed_llm_scheduler_amd/ops/gemm_tuning.json $O/orig.json
    cp distributed_llm_scheduler_amd/ops/gemm_tuning.json $O/refined.json
    DLS_GEMM_TUNING=$O/refined.json timeout -k 10 900 python benchmarks/refine_dag.py --model $m --reps ${REPS:-20} \
      > $O/refine.json 2> $O/refine.err || { tail -20 $O/refine.err; exit 4; }
    for i in 1 2; do
      for t in refined orig; do
        DLS_GEMM_TUNING=$O/$t.json timeout -k 10 300 python bench.py --model $m --steps 100 --warmup 5 --no-extras \
          > $O/b_$t.json 2>/dev/null || exit 5
        echo "$t $(ms $O/b_$t.json)"
      done
    done
    ;;
  stamps)
    : > $O/stamps.txt
    for shape in "24 512 2304 768" "27 512 768 768" "27 512 768 3072" "17 512 3072 768" "24 512 768 3072" "34 512 50304 768"; do
      timeout -k 5 30 gpubin/gemm_stamps $shape >> $O/stamps.txt 2>&1 || { echo "FAILED $shape"; exit 3; }
    done
    # the GPT-2 step's own configs, bare and with the epilogue operands the step attaches
    # (120..123: the wave-private rings, W x S = 8 x 2, 4 x 3, 6 x 2, 12 x 1, beside config 45)
    for shape in "45 512 768 768 res" "121 512 768 768 res" "122 512 768 768 res" "123 512 768 768 res" \
                 "45 512 768 3072 res" "120 512 768 3072 res" "121 512 768 3072 res" "122 512 768 3072 res" \
                 "123 512 768 3072 res" "17 512 2304 768 ln" "17 512 3072 768 lngelu" "13 512 50304 768 ln"; do
      s=($shape)
      for mode in none ${s[4]}; do
        timeout -k 5 30 gpubin/gemm_stamps ${s[0]} ${s[1]} ${s[2]} ${s[3]} $mode >> $O/stamps.txt 2>&1 || { echo "FAILED $shape $mode"; exit 3; }
      done
    done
    # the 64-row wave-private rings (130 / 131: 64 x 96 at W x S = 4 x 2 / 3 x 2; 132 / 133: 64 x 80),
    # which take the step's folded-norm operands only, beside config 17 above
    for shape in "130 512 3072 768 lngelu" "131 512 3072 768 lngelu" "132 512 3072 768 lngelu" "133 512 3072 768 lngelu" \
                 "130 512 2304 768 ln" "131 512 2304 768 ln" "132 512 2304 768 ln" "133 512 2304 768 ln"; do
      timeout -k 5 30 gpubin/gemm_stamps $shape >> $O/stamps.txt 2>&1 || { echo "FAILED $shape"; exit 3; }
    done
    cat $O/stamps.txt
    ;;
  prefill)
    # the first-token table and the chunk attention table, each a run of its own
    timeout -k 10 ${LIMIT:-500} python benchmarks/bench_prefill.py --skip-attention --out $O "$@" > $O/first_token.log 2>&1 \
      || { tail -20 $O/first_token.log; exit 3; }
    cat $O/first_token.txt
    timeout -k 10 ${LIMIT:-500} python benchmarks/bench_prefill.py --skip-ttft --out $O "$@" > $O/attn_chunk.log 2>&1 \
      || { tail -20 $O/attn_chunk.log; exit 4; }
    cat $O/attn_chunk_table.txt
    ;;
  moe-decode)
    # the kernel table and the step A/B, each a run of its own
    timeout -k 10 ${LIMIT:-500} python benchmarks/bench_moe_decode.py --out $O "$@" > $O/kernels.log 2>&1 \
      || { tail -20 $O/kernels.log; exit 3; }
    cat $O/kernels.txt
    timeout -k 10 ${LIMIT:-500} python benchmarks/bench_moe_decode.py --skip-kernels --step --out $O > $O/step.log 2>&1 \
      || { tail -20 $O/step.log; exit 4; }
    cat $O/step.txt
    ;;
  skinny)
    # the kernel table and the two step tables, each a run of its own
    timeout -k 10 ${LIMIT:-560} python benchmarks/bench_skinny.py --out $O "$@" > $O/kernels.log 2>&1 \
      || { tail -20 $O/kernels.log; exit 3; }
    cat $O/kernels.txt
    timeout -k 10 ${LIMIT:-400} python benchmarks/decode_step.py --skinny-gemm --out $O/step_llama3-8b-1l.txt > $O/step_llama.log 2>&1 \
      || { tail -20 $O/step_llama.log; exit 4; }
    cat $O/step_llama3-8b-1l.txt
    timeout -k 10 ${LIMIT:-300} python benchmarks/decode_step.py --skinny-gemm --model gpt2 --out $O/step_gpt2.txt > $O/step_gpt2.log 2>&1 \
      || { tail -20 $O/step_gpt2.log; exit 5; }
    cat $O/step_gpt2.txt
    ;;
  *)
    echo "unknown job $job"; exit 2
    ;;
esac
