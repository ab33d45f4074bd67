"""The fuzz of the opt-in stages at other seed bases (dev tool; the committed tests run twelve seeds per stage):

    python tools/fuzz_optin.py BASE COUNT [stage | table]

runs the cases (stage, BASE + 0 .. COUNT - 1) of tests/fuzz_scenes.py through tests/test_gpu_optin_fuzz.py's device calls --
every stage, or the one named -- and prints one line per case: the stage, the seed, the shape, the parameters, the form of
the call, and OK or the first difference; then `bad N`.  `table` is the table family of compositions instead: one context at
the shape of BASE, the cases BASE + 1 + 0 .. COUNT - 1 through PairPipeline and that context, then every case again on the same
context in the order fuzz_scenes.table_order gives (lines `table again`).  A HIP error ends the run at once (exit status 3):
nothing more is started on a device that has reported one.  Run from the repository root on the GPU box.
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np                             # noqa: E402

import fuzz_scenes as fs                       # noqa: E402
import oracle                                  # noqa: E402
import test_gpu_optin_fuzz as fuzz             # noqa: E402
from stereo_matching_cuda_amd import _lib      # noqa: E402


class DeviceError(Exception):
    pass


def one(label, text, call):
    """-> 1 for a mismatch, 0 for OK; DeviceError after the library's SMX_E_HIP or torch's own HIP error"""
    try:
        with np.errstate(all="ignore"):
            call()
        verdict = "OK"
    except AssertionError as e:
        verdict = "MISMATCH " + " ".join(str(e).split())[:300]
    except (_lib.SmxError, RuntimeError) as e:
        print(f"{label} {text}: ERROR {' '.join(str(e).split())[:300]}", flush=True)
        raise DeviceError
    print(f"{label} {text}: {verdict}", flush=True)
    return int(verdict != "OK")


def table(base, count):
    import stereo_matching_cuda_amd as smx
    bad = 0
    ctx = fuzz.create_table_context(base)
    try:
        for seed in range(count):
            bad += one(f"table {base}+{seed}", fs.table_composition(seed, base)["text"],
                       lambda: fuzz.run_table_composition(seed, ctx, oracle, base))
        for seed in fs.table_order(base, count):
            bad += one(f"table again {base}+{seed}", "", lambda: fuzz.run_table_again(seed, ctx, oracle, base))
    finally:
        smx.lib().smx_destroy(ctx)
    return bad


def main(argv):
    if len(argv) < 3 or (len(argv) > 3 and argv[3] not in fs.STAGES + ("table",)):
        print(__doc__)
        return 2
    base, count = int(argv[1]), int(argv[2])
    stages = [argv[3]] if len(argv) > 3 else list(fs.STAGES)
    oracle.build()
    bad = 0
    try:
        for stage in stages:
            t0 = time.time()
            if stage == "table":
                bad += table(base, count)
            for seed in range(count if stage != "table" else 0):
                bad += one(f"{stage} {base}+{seed}", fs.draw(stage, seed, base)["text"],
                           lambda: fuzz.run(stage, seed, base, orc=oracle))
            print(f"# {stage}: {count} cases in {time.time() - t0:.1f} s", flush=True)
    except DeviceError:
        print("stopped: no further case on a device that reported an error")
        print("bad", bad + 1)
        return 3
    print("bad", bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
