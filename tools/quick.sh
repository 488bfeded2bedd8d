#!/bin/bash
# One quick GPU check of the current tree: the -m gpu suite, then the default bench line (no CPU
# leg, no extras).  Usage: tools/quick.sh TAG [bench args...]
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
tag=${1:-q}; shift || true
out=${COEB_OUT_DIR:-out}/$tag       # where the logs go
mkdir -p "$out"
export TMPDIR=/tmp
timeout -k 10 300 python -u -m pytest tests -q -m gpu -x --timeout 120 --timeout-method thread > $out/pytest.log 2>&1
rc=$?; tail -n 3 $out/pytest.log
[ $rc -ne 0 ] && { grep -E "Error|assert|FAILED" $out/pytest.log | head -20; exit $rc; }
timeout -k 10 300 python bench.py --full --no-cpu-baseline --no-extras "$@" > $out/bench.log 2>&1
rc=$?
python - "$out/bench.log" <<'PY'
import json, sys
for l in open(sys.argv[1]):
    if l.startswith("{"):
        d = json.loads(l)
        print("value", d["value"], "ms/step", d["ms_per_step"], "kernels", d.get("kernels_ms_per_step"))
PY
exit $rc
