"""What tests/test_oracle_ref.py and tests/test_gpu_ref_cases.py share: the recorded results of the reference's own code
(tests/golden/ref_cases/<name>.npz, written by oracle/ref_build.py) and the comparison with them.  Reads neither the reference
nor oracle/_ref."""
import ctypes as C
import json
import os

import numpy as np

from oracle import ref_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "golden", "ref_cases")
NAMES = sorted(f[:-4] for f in os.listdir(DIR) if f.endswith(".npz")) if os.path.isdir(DIR) else []


def names(mode):
    return [n for n in NAMES if n in rc.BY_NAME and rc.BY_NAME[n]["mode"] == mode]


def load(name):
    """(case of the table, fixture arrays).  The fixture was recorded for exactly the table's case."""
    fx = dict(np.load(os.path.join(DIR, name + ".npz")))
    c = rc.BY_NAME[name]
    recorded = json.loads(str(fx.pop("case")))
    assert recorded == json.loads(json.dumps({k: c[k] for k in c if k != "axes"})), f"{name}: the fixture was recorded for another case"
    return c, fx


def inputs(c):
    needs = load(c["needs"])[1] if c.get("needs") else None
    return rc.inputs(c, needs)


def set_params(p, m):
    """smx_params / orc_params (the same layout) from a macro set."""
    p.alpha, p.th_color, p.th_grad = float(m["ALPHA"]), int(m["TH_color"]), int(m["TH_grad"])
    p.radius, p.eps, p.d_lr = int(m["RADIUS"]), float(m["EPS"]), int(m["D_LR"])
    return p


def first_difference(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float32:
        both_nan = np.isnan(a) & np.isnan(b)
        a = np.where(both_nan, 0, a.view(np.uint32))
        b = np.where(both_nan, 0, b.view(np.uint32))
    bad = np.argwhere(a != b)
    return f"{len(bad)} of {a.size} elements differ, first at {bad[:5].tolist()}"


def compare(name, fx, got, what="", locate=None):
    """Every array of `got` the fixture holds must be the fixture's: maps bit for bit (both-NaN counts as equal, like _eq of
    tests/test_gpu_parity.py), hashed arrays by the sha256 of their bytes with NaN canonicalised.  locate(key) may return the
    full recorded array of a hashed key, to say where a difference is.  Returns the keys compared."""
    seen = []
    for key, a in got.items():
        if key in fx:
            want = fx[key]
            a = np.asarray(a)
            assert a.shape == want.shape and a.dtype == want.dtype, (name, what, key, a.shape, want.shape, a.dtype, want.dtype)
            assert rc.sha256_canonical(a) == rc.sha256_canonical(want), f"{name} {what} {key}: {first_difference(a, want)}"
        elif "sha_" + key in fx:
            if rc.sha256_canonical(a) != str(fx["sha_" + key]):
                full = locate(key) if locate else None
                where = first_difference(np.asarray(a).reshape(full.shape), full) if full is not None else "no full copy recorded"
                raise AssertionError(f"{name} {what} {key}: sha256 differs from the reference's ({where})")
        else:
            continue
        seen.append(key)
    return seen


def expect_all(fx, seen, but=()):
    """Nothing the fixture holds went unchecked."""
    have = {k[4:] if k.startswith("sha_") else k for k in fx}
    assert have - set(but) <= set(seen), sorted(have - set(but) - set(seen))


def byref_default(cls, lib_default):
    p = cls()
    lib_default(C.byref(p))
    return p
