"""Developer tool: the inputs of tests/test_gpu_front_chain.py through the instrumented build of the front gapped kernel
(`make -C priblast_amd/csrc prof` -> libpriblast_hip_prof.so; needs a GPU): per case the hit counts, the launches and the
kernel's counters - cells, pairs, directions given up, cells whose candidate scan takes a second / third batch, cells of a
direction with one record's room left, cells behind a wobble pair, steps that outgrow the cell list or the pool.  The figures in
that file's docstring come from here; run it again when gen_synthetic, the seeds or the kernel's constants change."""
import ctypes
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from priblast_amd import capi  # noqa: E402

capi.LIB_PATH = os.path.join(ROOT, "priblast_amd", "lib", "libpriblast_hip_prof.so")
import test_gpu_front_chain as T  # noqa: E402


def main():
    ctx = capi.Context(0)
    L = capi.lib()
    buf = (ctypes.c_ulonglong * 32)()
    for case, spec in T.CASES.items():
        qs, names, seqs = spec[0]()
        opts = {"final_threshold": spec[3]} if len(spec) > 3 else {}
        d = tempfile.mkdtemp(prefix="front_cases_")
        capi.db_build(ctx, d + "/db", names, seqs, 0, 8, 70, 5)
        db = capi.Db(ctx, d + "/db")
        qb = capi.QBatch(ctx, qs, db.repeat_flag)
        qb.accessibility(db.W, db.delta)
        L.prb_debug_front_profile(buf, 1)
        ctx.reset_timers()
        _, _, c = capi.search_page(ctx, qb, db, 0, capi.default_opts(output_style=1, **opts))
        L.prb_debug_front_profile(buf, 1)
        v = list(buf)
        print(f"{case}: counts {tuple(c)} launches {ctx.stage_ms('gapped_front')[1]} | tiles {v[16]} steps {v[17]} cells {v[19]} pairs {v[20]} | "
              f"given up: more than a direction's cells {v[21]}, improved {v[22]} | scan: second batch {v[27]}, third {v[28]}, one record's room left {v[29]} | "
              f"cells behind a wobble pair {v[30]} | steps that outgrow the cell list or the pool {v[31]}", flush=True)
        qb.close()
        db.close()


if __name__ == "__main__":
    main()
