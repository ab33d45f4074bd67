"""The fuzz of the opt-in stages at other seed bases (dev tool; the committed tests run twelve seeds per stage):

    python tools/fuzz_optin.py BASE COUNT [stage]

runs the cases (stage, BASE + 0 .. COUNT - 1) of tests/fuzz_scenes.py through tests/test_gpu_optin_fuzz.py's device calls --
every stage, or the one named -- and prints one line per case: the stage, the seed, the shape, the parameters, the form of
the call, and OK or the first difference; then `bad N`.  A HIP error ends the run at once (exit status 3): nothing more is
started on a device that has reported one.  Run from the repository root on the GPU box.
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import fuzz_scenes as fs                       # noqa: E402
import oracle                                  # noqa: E402
import test_gpu_optin_fuzz as fuzz             # noqa: E402
from stereo_matching_cuda_amd import _lib      # noqa: E402


def main(argv):
    if len(argv) < 3 or (len(argv) > 3 and argv[3] not in fs.STAGES):
        print(__doc__)
        return 2
    base, count = int(argv[1]), int(argv[2])
    stages = [argv[3]] if len(argv) > 3 else list(fs.STAGES)
    oracle.build()
    bad = 0
    for stage in stages:
        t0 = time.time()
        for seed in range(count):
            text = fs.draw(stage, seed, base)["text"]
            try:
                fuzz.run(stage, seed, base, orc=oracle)
                verdict = "OK"
            except AssertionError as e:
                bad += 1
                verdict = "MISMATCH " + " ".join(str(e).split())[:300]
            except (_lib.SmxError, RuntimeError) as e:          # the library's SMX_E_HIP, or torch's own HIP error
                print(f"{stage} {base}+{seed} {text}: ERROR {' '.join(str(e).split())[:300]}", flush=True)
                print("stopped: no further case on a device that reported an error")
                print("bad", bad + 1)
                return 3
            print(f"{stage} {base}+{seed} {text}: {verdict}", flush=True)
        print(f"# {stage}: {count} cases in {time.time() - t0:.1f} s", flush=True)
    print("bad", bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
