# Bench the default library under environment-variable variants: args "NAME=VAL" or "base".
set -u
cd "${GRAFT_REPO_ROOT:-.}"
out=${COEB_OUT_DIR:-out}       # where the logs go
mkdir -p "$out"
for v in "$@"; do
  if [ "$v" = base ]; then envs=""; else envs="$v"; fi
  env $envs timeout -k 10 300 python bench.py --full --no-cpu-baseline --no-e2e --steps 10 > $out/env.log 2>&1 || { echo "variant $v failed rc=$?"; tail -5 $out/env.log; exit 1; }
  python - "$v" $out/env.log <<'PY'
import json, sys
d = json.loads([l for l in open(sys.argv[2]) if l.startswith("{")][-1])
print("[%s] value=%.0f ms/step=%.4f kernels=%s" % (sys.argv[1], d["value"], d["ms_per_step"], d["kernels_ms_per_step"]))
PY
done
