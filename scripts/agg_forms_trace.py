"""Every case of tests/test_gpu_agg_forms.py once, in one process, for a kernel trace of the sink forms:
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o p -- python3 scripts/agg_forms_trace.py
The kind assertions are made when the library reports a kind (a commit before ph_agg_sink_kind runs the same sinks without them), so
the traces of two commits compare launch for launch. PH_AGG_NO_BULK and PH_AGG_BULK_V1 were once read at a process's first sink only:
their cases are left out so that both sides run the same sinks."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_gpu_agg_forms as T  # noqa: E402
from plan_amd import hip  # noqa: E402

ONCE_PER_PROCESS = {"PH_AGG_NO_BULK", "PH_AGG_BULK_V1"}


def main():
    says_kind = hasattr(hip.Agg, "sink_kind")
    ctx, rows = hip.Ctx(0), T.Rows()
    for name, n, hint, env, distinct, kind in T.CASES:
        if ONCE_PER_PROCESS & set(env):
            continue
        for k in T.SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(env)
        T.sink_and_check(ctx, rows, n, hint, distinct, kind if says_kind else None)
        print(f"{name}: {n} rows, hint {hint}: {kind if says_kind else 'groups'} ok", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
