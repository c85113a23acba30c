#!/bin/bash
# enwik9-like compress throughput against blocks in flight (corpus generated once)
cd "$(dirname "$0")/.."
export JAMPACK_CORPUS_CACHE=/tmp/jpk_corpus
CS=${CS:-"4 8 12 15"}
for c in $CS; do
  python bench.py --workload enwik9 --contexts $c --steps 2 --warmup 1 --no-extras 2>/dev/null | python -c "import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('contexts $c:', d['value'], 'MB/s', d['ms_per_step'], 'ms')"
done
