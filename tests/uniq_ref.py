"""numpy reference of the uniqueness (peak-ratio) filter (include/smx.h: smx_dev_aggregate_wta_pair_uq, smx_dev_sgm_wta_pair_uq,
smx_dev_uniqueness), float32 throughout.

From an aggregated volume q[D][h][w] and the slice range [s_begin, s_end) that was aggregated:
  second_best   the winner by the key's rules (smallest cost, the LAST slice among equal costs, a NaN never wins) and, BY THE
                DEFINITION, sec = min { q(k) : |k - z*| >= 2, q(k) not NaN } (+inf if there is none), rest = the min over all
                slices but the last, last = the last slice's cost.  Every min is one ascending scan from +inf that takes a value
                only where it is strictly smaller, which fixes the bits among equal values (-0 == +0: the first stays).
  emulate       the streaming recurrence of the kernels (smx_common.h WtaRunUq) pixel by pixel in plain Python, over arbitrary
                chunk splits, each chunk resumed from the packed key and the stored state.
  margin, rejects, counts, apply    the test and the filtered map.
"""
import numpy as np

F32 = np.float32
INF = F32(np.inf)
NAN = F32(np.nan)
IDENT = np.iinfo(np.int64).max


# ---- the packed key (smx_common.h pack_key / unpack_key) ----------------------------------------------------------------
def pack_key(cost, slice_):
    cost = F32(cost)
    if np.isnan(cost):
        return IDENT
    if cost == 0:
        cost = F32(0.0)
    u = int(np.array(cost, F32).view(np.uint32))
    if u & 0x80000000:
        u = (~u ^ 0x80000000) & 0xFFFFFFFF
    k = (u << 32) | (0xFFFFFFFF - int(slice_))
    return k - (1 << 64) if k >= (1 << 63) else k


def unpack_key(key):
    k = int(key) & 0xFFFFFFFFFFFFFFFF
    u = k >> 32
    if u & 0x80000000:
        u = ~(u ^ 0x80000000) & 0xFFFFFFFF
    return np.array(u, np.uint32).view(F32)[()], 0xFFFFFFFF - (k & 0xFFFFFFFF)


def pack_keys(c0, z):
    """vectorised: the keys of winners (z, c0); z < 0 gives the identity."""
    c0 = np.asarray(c0, F32)
    c = np.where(c0 == 0, F32(0), c0).astype(F32)
    u = c.view(np.uint32).astype(np.uint64)
    u = np.where(u & np.uint64(0x80000000), (~u ^ np.uint64(0x80000000)) & np.uint64(0xFFFFFFFF), u)
    k = (u << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.maximum(z, 0).astype(np.uint64))
    return np.where((np.asarray(z) >= 0) & ~np.isnan(c0), k.view(np.int64), IDENT)


# ---- the definition ------------------------------------------------------------------------------------------------------
def _scan_min(v, eligible):
    """ascending scan from +inf over v[k] where eligible[k]: strictly smaller values only (a NaN compares false)"""
    out = np.full(v.shape[1:], INF, F32)
    with np.errstate(invalid="ignore"):
        for k in range(v.shape[0]):
            out = np.where(eligible[k] & (v[k] < out), v[k], out)
    return out.astype(F32)


def second_best(q, s_begin=0, s_end=None):
    """-> (z, c0, sec, rest, last, zsec): z the absolute winning slice (-1: none), c0 its cost with -0 folded to +0 (the key's),
    sec / rest / last as above, zsec the absolute slice sec was taken from (-1: none)."""
    q = np.asarray(q, F32)
    s_end = q.shape[0] if s_end is None else s_end
    v = q[s_begin:s_end]
    n = v.shape[0]
    nan = np.isnan(v)
    has = ~nan.all(axis=0)
    m = np.where(nan, INF, v).min(axis=0)
    hit = (v == m[None]) & ~nan
    k = n - 1 - np.argmax(hit[::-1], axis=0)                      # the last slice of the minimum
    z = np.where(has, s_begin + k, -1)
    kk = np.where(has, k, 0)
    c0 = np.take_along_axis(v, kk[None], 0)[0]
    c0 = np.where(has, np.where(c0 == 0, F32(0), c0), NAN).astype(F32)
    idx = np.arange(n).reshape((n,) + (1,) * (v.ndim - 1))
    far = has[None] & (np.abs(idx - kk[None]) >= 2)
    sec = _scan_min(v, far)
    with np.errstate(invalid="ignore"):
        first = np.argmax(far & (v == sec[None]) & ~nan, axis=0)
    zsec = np.where(sec < INF, s_begin + first, -1)
    rest = _scan_min(v[:-1], np.ones(v[:-1].shape, bool)) if n > 1 else np.full(v.shape[1:], INF, F32)
    return z, c0, sec, rest, v[-1].copy(), zsec


# ---- the streaming form ----------------------------------------------------------------------------------------------------
def step(state, v, z):
    """one slice of WtaRunUq: state = [m, zs, sec, rest, last] (zs = -1: no winner yet), cost v at absolute slice z"""
    m, zs, sec, rest, last = state
    v = F32(v)
    with np.errstate(invalid="ignore"):
        take = bool(v <= m)
        if take:
            sec = rest
        elif zs >= 0 and z >= zs + 2 and bool(v < sec):
            sec = v
        if take:
            m, zs = v, z
        if bool(last < rest):
            rest = last
    return [m, zs, sec, rest, v]


def emulate(col, chunks, s_begin=0):
    """One pixel's costs col[0 ..] (slices s_begin ..) in chunks of the given lengths (sum == len(col)); every chunk starts
    from the packed key and the stored (sec, rest, last) of the one before, as a launch does.
    -> (key, sec, rest, last, trace) with trace = [(first slice, last slice, winner slice after the chunk), ...]."""
    assert sum(chunks) == len(col)
    key, stored = IDENT, (F32(123.0), F32(-7.0), F32(55.0))      # (an identity key: the stored state is not read)
    at, trace = 0, []
    for n in chunks:
        if key == IDENT:
            state = [INF, -1, INF, INF, NAN]
        else:
            c, zs = unpack_key(key)
            state = [c, zs, stored[0], stored[1], stored[2]]
        for i in range(at, at + n):
            state = step(state, col[i], s_begin + i)
        key = IDENT if state[1] < 0 else pack_key(state[0], state[1])
        stored = (state[2], state[3], state[4])
        trace.append((s_begin + at, s_begin + at + n - 1, state[1]))
        at += n
    return key, F32(stored[0]), F32(stored[1]), F32(stored[2]), trace


def splits(n):
    """every split of n slices into consecutive chunks (2^(n-1) of them)"""
    if n == 0:
        return [[]]
    out = []
    for mask in range(1 << (n - 1)):
        cuts, run = [], 1
        for b in range(n - 1):
            if mask >> b & 1:
                cuts.append(run)
                run = 1
            else:
                run += 1
        out.append(cuts + [run])
    return out


# ---- the test ---------------------------------------------------------------------------------------------------------------
def margin(has, c0, sec):
    """s - c0; +inf where s is unknown (+inf, NaN); NaN where the key is the identity"""
    c0, sec = np.asarray(c0, F32), np.asarray(sec, F32)
    with np.errstate(invalid="ignore"):
        known = sec < INF
        d = (sec - c0).astype(F32)
    return np.where(has, np.where(known, d, INF), NAN).astype(F32)


def rejects(has, c0, sec, ratio):
    """rejected iff the key is not the identity, ratio > 0 and s - c0 < ratio * |c0| (f32, each operation rounded on its own)"""
    c0, sec = np.asarray(c0, F32), np.asarray(sec, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        known = sec < INF
        d = (sec - c0).astype(F32)
        bound = (F32(ratio) * np.abs(c0)).astype(F32)
        return np.asarray(has) & known & (F32(ratio) > 0) & (d < bound)


def counts(disp, vmin):
    """the speckle filter's validity rule: finite and (float)(int)disp >= vmin with the saturating truncation toward zero"""
    d = np.asarray(disp, F32)
    fin = np.isfinite(d)
    t = np.clip(np.trunc(np.where(fin, d, 0).astype(np.float64)), -2147483648.0, 2147483648.0).astype(F32)
    return fin & (t >= F32(vmin))


def apply(disp, has, c0, sec, ratio, vmin, new_val):
    """-> (filtered map, margin)"""
    d = np.asarray(disp, F32)
    rej = rejects(has, c0, sec, ratio) & counts(d, vmin)
    return np.where(rej, F32(new_val), d).astype(F32), margin(has, c0, sec)


def key_fields(keys):
    """(has, c0) of an array of packed keys"""
    keys = np.asarray(keys, np.int64)
    has = keys != IDENT
    u = (keys.view(np.uint64) >> np.uint64(32)).astype(np.uint32)
    u = np.where(u & np.uint32(0x80000000), ~(u ^ np.uint32(0x80000000)), u).astype(np.uint32)
    return has, np.where(has, u.view(F32), NAN).astype(F32)
