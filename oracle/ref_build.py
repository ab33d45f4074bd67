"""Builds the reference itself as host programs and records what it computes for every case of oracle/ref_cases.py.
TEST INFRASTRUCTURE ONLY; everything it makes goes under oracle/_ref/ (git-ignored).

The reference (hamza1030/stereo_matching_cuda, CUDA) is read from $SMX_REFERENCE_DIR (default /root/reference).  Where that
directory is absent this script prints one line and succeeds, leaving an existing oracle/_ref/ as it is.

Per macro set of the case table (ref_cases.VARIANTS):
  1. copy the six translation units behind the five pinned host functions (costVolume, guidedFilter, helpers, integral,
     occlusion, rgb_to_grayscale: .cu), every .cuh and SystemIncludes.h to oracle/_ref/src_<variant>/.  main.cu, filter.cu
     (dead code with shared-memory tile kernels), the stb headers and the images are not copied.  Of main.cu only the text
     of write_mat (main.cu:13-35, the float -> 8-bit normaliser in front of the PNG writer) is cut out into a unit of its own,
     write_mat.cu, behind the stbi_write_png stand-in of oracle/ref_shim/stb_image_write.h;
  2. rewrite every `kernel<<<grid, block>>>(args);` to `LAUNCH(kernel, grid, block, args);` (oracle/ref_shim/cuda_runtime.h:
     serial thread loop, refused for every kernel not known to be exact under it -- the list is in that header);
  3. rewrite the #define lines of SystemIncludes.h to the macro set;
  4. add `ref_capture_q(d_q, n);` after the compute_q launch (guidedFilter.cu:233): the aggregated volume, which the reference
     never keeps, is appended plane by plane to a file the driver opens;
  5. compile with g++ -O2 -ffp-contract=off -fno-fast-math and link oracle/ref_driver.cpp -> oracle/_ref/ref_<variant>;
     the same again with -fsanitize=address,undefined -fno-sanitize-recover=all -> oracle/_ref/ref_<variant>_san.
Then every case runs through the sanitized program first.  A case in which the reference itself reads or writes out of bounds
or overflows an int has no defined answer: it gets no fixture, and its evidence goes to oracle/_ref/excluded/<name>.txt (the
committed list is oracle/REF_CASES.md).  Every other case runs through the plain program and is recorded to
oracle/_ref/fixtures/<name>.npz; small cases keep their full volumes in oracle/_ref/cases/<name>.npz.

    python oracle/ref_build.py                    build + record (a second call does nothing: oracle/_ref/STAMP)
    python oracle/ref_build.py --write-fixtures   also copy the recorded fixtures to tests/golden/ref_cases/
"""
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import ref_cases as rc  # noqa: E402

REF = os.path.join(HERE, "_ref")
FIXTURES = os.path.join(ROOT, "tests", "golden", "ref_cases")
UNITS = ("costVolume", "guidedFilter", "helpers", "integral", "occlusion", "rgb_to_grayscale")
RECIPE = ("ref_build.py", "ref_cases.py", "ref_driver.cpp", "ref_shim/cuda_runtime.h", "ref_shim/device_launch_parameters.h",
          "ref_shim/shim.cpp", "ref_shim/stb_image_write.h")
WRITE_MAT_RE = re.compile(r"^void write_mat\([^)]*\) \{\n.*?^\}\n", re.M | re.S)
JOBS = min(16, os.cpu_count() or 1)
FLAGS = ["-ffp-contract=off", "-fno-fast-math", "-w", "-std=c++14"]
FLAVOURS = {"": ["-O2"], "_san": ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                                  "-fsanitize=float-cast-overflow", "-fno-sanitize-recover=all"]}
# Two reports of AddressSanitizer that are neither an access out of bounds nor an overflow are switched off, on every case alike:
# integralOnCPU frees a new[] block with free() (integral.cu:94, :118: alloc-dealloc-mismatch), and detect_occlusion never
# frees two host buffers (occlusion.cu:21-22: leak).
SAN_ENV = {"ASAN_OPTIONS": "detect_leaks=0:alloc_dealloc_mismatch=0:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"}
KEEP_VOLUMES_BELOW = 4 << 20           # bytes of all volumes of a case; oracle/_ref travels with the tree
LAUNCH_RE = re.compile(r"^([ \t]*)(\w+)\s*<<\s*<\s*(\w+)\s*,\s*(\w+)\s*>>\s*>\s*\((.*?)\);", re.M | re.S)


def reference_dir():
    d = os.path.join(os.environ.get("SMX_REFERENCE_DIR", "/root/reference"), "stereo_matching_cuda")
    return d if os.path.isfile(os.path.join(d, "SystemIncludes.h")) and os.access(d, os.R_OK | os.X_OK) else None


def _reference_files(ref):
    return sorted(f for f in os.listdir(ref) if f.endswith(".cuh") or f == "SystemIncludes.h" or f[:-3] in UNITS and f.endswith(".cu"))


def _write_mat_unit(ref):
    """write_mat of main.cu as a translation unit: the function's own text between two lines of ours."""
    text = open(os.path.join(ref, "main.cu"), encoding="utf-8", errors="surrogateescape").read()
    found = WRITE_MAT_RE.findall(text)
    assert len(found) == 1 and "main(" not in found[0] and found[0].count("stbi_write_png(") == 1, found
    return '#include <cstdlib>\n#include <cstring>\n#include "stb_image_write.h"\n\n' + found[0]


def stamp_of(ref):
    h = hashlib.sha256()
    for f in RECIPE:
        h.update(open(os.path.join(HERE, f), "rb").read())
    for f in _reference_files(ref):
        h.update(f.encode())
        h.update(open(os.path.join(ref, f), "rb").read())
    h.update(_write_mat_unit(ref).encode("utf-8", errors="surrogateescape"))
    h.update(open(os.path.join(ROOT, "tests", "golden", "tsukuba_golden.npz"), "rb").read())
    return h.hexdigest()


def is_current(ref):
    try:
        done = json.load(open(os.path.join(REF, "STAMP")))
    except (OSError, ValueError):
        return False
    return (done.get("stamp") == stamp_of(ref) and
            all(os.path.exists(os.path.join(REF, "fixtures", n + ".npz")) for n in done["kept"]) and
            all(os.path.exists(os.path.join(REF, "ref_" + v)) for v in rc.VARIANTS))


# ---- the temporary copies ----------------------------------------------------------------------------------------------
def _prepare_sources(ref, name, m):
    src = os.path.join(REF, "src_" + name)
    shutil.rmtree(src, ignore_errors=True)
    os.makedirs(src)
    for f in _reference_files(ref):
        text = open(os.path.join(ref, f), encoding="utf-8", errors="surrogateescape").read()
        if f.endswith(".cu"):
            text = LAUNCH_RE.sub(r"\1LAUNCH(\2, \3, \4, \5);", text)
            left = [ln for ln in text.splitlines() if re.search(r"<<\s*<", ln) and not ln.lstrip().startswith("//")]
            assert not left, (f, left)
        if f == "guidedFilter.cu":
            text, k = re.subn(r"^([ \t]*)(LAUNCH\(compute_q,[^;]*;)", r"\1\2\n\1ref_capture_q(d_q, n);", text, flags=re.M)
            assert k == 1, k
        if f == "SystemIncludes.h":
            for key in rc.MACRO_ORDER:
                text, k = re.subn(rf"^#define {key}[ \t]+\S.*$", f"#define {key} {rc.macro_text(key, m[key])}", text, flags=re.M)
                assert k == 1, (key, k)
        with open(os.path.join(src, f), "w", encoding="utf-8", errors="surrogateescape") as out:
            out.write(text)
    with open(os.path.join(src, "write_mat.cu"), "w", encoding="utf-8", errors="surrogateescape") as out:
        out.write(_write_mat_unit(ref))
    return src


def _run(cmd, **kw):
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, **kw)
    return p.returncode, p.stdout.decode(errors="replace")


def _compile(job):
    out, src_file, inc, flags = job
    rcode, log = _run(["g++", *FLAGS, *flags, "-x", "c++", "-I" + os.path.join(HERE, "ref_shim"), "-I" + inc, "-c", src_file, "-o", out])
    if rcode:
        raise RuntimeError(f"g++ failed on {src_file}:\n{log}")
    return out


def build_programs(ref, pool):
    jobs, links = [], []
    for name, m in rc.VARIANTS.items():
        src = _prepare_sources(ref, name, m)
        for flavour, flags in FLAVOURS.items():
            objs = []
            units = [os.path.join(src, u + ".cu") for u in UNITS + ("write_mat",)] + [os.path.join(HERE, "ref_driver.cpp"),
                                                                     os.path.join(HERE, "ref_shim", "shim.cpp")]
            for u in units:
                o = os.path.join(src, os.path.basename(u) + flavour + ".o")
                jobs.append((o, u, src, flags))
                objs.append(o)
            links.append((os.path.join(REF, "ref_" + name + flavour), objs, flags))
    list(pool.map(_compile, jobs))

    def link(job):
        exe, objs, flags = job
        rcode, log = _run(["g++", *[f for f in flags if f.startswith("-fsanitize") or f.startswith("-fno-sanitize")], *objs, "-o", exe])
        if rcode:
            raise RuntimeError(f"link of {exe} failed:\n{log}")
    list(pool.map(link, links))
    for name in rc.VARIANTS:                       # the objects are not needed again
        for f in os.listdir(os.path.join(REF, "src_" + name)):
            if f.endswith(".o"):
                os.remove(os.path.join(REF, "src_" + name, f))


# ---- running the cases -------------------------------------------------------------------------------------------------
def _write_inputs(c, rundir, needs):
    for stem, a in rc.inputs(c, needs).items():
        ext = ".f32" if a.dtype == np.float32 else ".u8"
        np.ascontiguousarray(a).tofile(os.path.join(rundir, stem + ext))


def _read_outputs(c, rundir):
    w, h = c["w"], c["h"]
    out = {}
    for key, (fname, dt, _) in rc.OUTPUTS[c["mode"]].items():
        p = os.path.join(rundir, fname)
        if os.path.exists(p):
            a = np.fromfile(p, dtype=dt)
            out[key] = a.reshape(-1, h, w) if a.size != w * h else a.reshape(h, w)
    return out


def run_case(c, needs=None):
    """(fixture dict, volumes dict) of a kept case, or (None, evidence text) of one the reference has no defined answer for."""
    name, var = c["name"], rc.variant(c["macros"])
    rundir = os.path.join(REF, "run", name)
    results = []
    for flavour in ("_san", ""):
        shutil.rmtree(rundir, ignore_errors=True)
        os.makedirs(rundir)
        _write_inputs(c, rundir, needs)
        cmd = [os.path.join(REF, "ref_" + var + flavour), c["mode"], rundir, *map(str, rc.driver_args(c))]
        rcode, log = _run(cmd, env=dict(os.environ, **SAN_ENV))
        if rcode:
            if flavour == "_san" and ("Sanitizer" in log or "runtime error" in log):
                shutil.rmtree(rundir, ignore_errors=True)
                return None, f"$ {' '.join(os.path.relpath(x, ROOT) if os.path.isabs(x) else x for x in cmd)}\nexit {rcode}\n{log}"
            raise RuntimeError(f"case {name}: {cmd} failed with {rcode}:\n{log[-4000:]}")
        results.append(_read_outputs(c, rundir))
    shutil.rmtree(rundir, ignore_errors=True)
    san, plain = results
    for k in plain:                                 # -O1 with sanitizers and -O2 without: the same IEEE arithmetic
        assert rc.sha256_canonical(san[k]) == rc.sha256_canonical(plain[k]), (name, k, "sanitized and plain builds differ")
    outputs = rc.OUTPUTS[c["mode"]]
    fixture = {"case": np.array(json.dumps({k: c[k] for k in c if k != "axes"}, sort_keys=True))}
    volumes = {}
    for k, a in plain.items():
        if outputs[k][2] or k in c.get("hash_only", ()):
            fixture["sha_" + k] = np.array(rc.sha256_canonical(a))
            if outputs[k][2]:
                volumes[k] = a
        else:
            fixture[k] = a
    return fixture, volumes


def record(pool):
    for d in ("fixtures", "cases", "excluded", "run"):
        shutil.rmtree(os.path.join(REF, d), ignore_errors=True)
        os.makedirs(os.path.join(REF, d))
    kept, excluded = {}, {}

    def one(c):
        needs = kept[c["needs"]] if c.get("needs") else None
        return c, run_case(c, needs)

    first = [c for c in rc.CASES if not c.get("needs")]
    second = [c for c in rc.CASES if c.get("needs")]
    for batch in (first, second):
        for c, (fixture, rest) in pool.map(one, batch):
            name = c["name"]
            if fixture is None:
                excluded[name] = rest
                open(os.path.join(REF, "excluded", name + ".txt"), "w").write(rest)
                continue
            kept[name] = fixture
            np.savez_compressed(os.path.join(REF, "fixtures", name + ".npz"), **fixture)
            if rest and sum(a.nbytes for a in rest.values()) < KEEP_VOLUMES_BELOW:
                np.savez(os.path.join(REF, "cases", name + ".npz"), **rest)
    shutil.rmtree(os.path.join(REF, "run"), ignore_errors=True)
    return kept, excluded


def write_fixtures():
    os.makedirs(FIXTURES, exist_ok=True)
    for f in os.listdir(FIXTURES):
        if f.endswith(".npz"):
            os.remove(os.path.join(FIXTURES, f))
    for f in sorted(os.listdir(os.path.join(REF, "fixtures"))):
        shutil.copyfile(os.path.join(REF, "fixtures", f), os.path.join(FIXTURES, f))


def main(argv=()):
    ref = reference_dir()
    if ref is None:
        print("oracle/ref_build.py: no reference at $SMX_REFERENCE_DIR (default /root/reference): oracle/_ref is left as it is")
        return 0
    if not is_current(ref):
        os.makedirs(REF, exist_ok=True)
        if os.path.exists(os.path.join(REF, "STAMP")):
            os.remove(os.path.join(REF, "STAMP"))
        with ThreadPoolExecutor(JOBS) as pool:
            build_programs(ref, pool)
            kept, excluded = record(pool)
        json.dump({"stamp": stamp_of(ref), "kept": sorted(kept), "excluded": sorted(excluded)},
                  open(os.path.join(REF, "STAMP"), "w"), indent=1)
        print(f"oracle/ref_build.py: {len(rc.VARIANTS)} builds of the reference, {len(kept)} cases recorded, "
              f"{len(excluded)} without a defined answer: {' '.join(sorted(excluded))}")
    if "--write-fixtures" in argv:
        write_fixtures()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
