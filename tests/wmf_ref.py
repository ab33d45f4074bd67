"""numpy reference of the weighted-median refinement (include/smx.h smx_weighted_median).

Not a test module: the tests of the stage import it.  The oracle under oracle/ has no such stage (the reference has
none), so this is the reference the GPU results are held against bit for bit.  `weighted_median` is vectorised over
pixels -- one pass per window offset, label histograms in bounded row bands -- and `brute_force` is the per-pixel
loop it is checked against on tiny images.
"""
import numpy as np


def weight_tables(radius, sigma_s, sigma_c):
    """The contract's formula in double: spatial[k], k = 0 .. 2 r^2, and range[t], t = 0 .. 255 (uint16)."""
    k = np.arange(2 * radius * radius + 1, dtype=np.float64)
    t = np.arange(256, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        ws = np.floor(1023.0 * np.exp(-k / (sigma_s * sigma_s)) + 0.5)
        wc = np.floor(1023.0 * np.exp(-(t * t) / (sigma_c * sigma_c)) + 0.5)
    ws[0] = wc[0] = 1023
    return ws.astype(np.uint16), wc.astype(np.uint16)


def labels(disp, dmin, size_d):
    """Label index (disp - dmin) of every pixel, -1 where the value counts for nothing."""
    d = np.asarray(disp, np.float32).astype(np.float64)
    ok = np.isfinite(d) & (np.abs(d) < 2.0 ** 31)
    di = np.where(ok, d, 0.0)
    ok &= np.trunc(di) == di
    k = np.where(ok, di, 0.0).astype(np.int64) - int(dmin)
    ok &= (k >= 0) & (k < size_d)
    return np.where(ok, k, -1)


def selected(select, dmin, shape):
    """Pixels that are filtered: all when select is None, else (int)select < dmin; NaN / +-inf select nothing."""
    if select is None:
        return np.ones(shape, bool)
    s = np.asarray(select, np.float32).astype(np.float64)
    fin = np.isfinite(s)
    return fin & (np.trunc(np.where(fin, s, 0.0)) < dmin)


def _result(disp, dmin, kstar, total):
    return np.where(total > 0, (int(dmin) + kstar).astype(np.float32), disp)


def weighted_median(guide, disp, dmin, size_d, select=None, radius=9, spatial=None, rng=None, band_elems=1 << 22):
    """Vectorised reference.  spatial / rng: the weight tables (default: weight_tables with the default sigmas)."""
    disp = np.ascontiguousarray(disp, np.float32)
    h, w = disp.shape
    if spatial is None or rng is None:
        spatial, rng = weight_tables(radius, 9.0, 25.5)
    ws = np.asarray(spatial, np.int64)
    wc = np.asarray(rng, np.int64)
    k = labels(disp, dmin, size_d)
    g = np.asarray(guide, np.int64)
    sel = selected(select, dmin, disp.shape)
    out = disp.copy()
    band = max(1, min(h, band_elems // (w * size_d)))
    for y0 in range(0, h, band):
        y1 = min(h, y0 + band)
        if not sel[y0:y1].any():
            continue
        bh = y1 - y0
        hist = np.zeros((bh, w, size_d), np.int64)
        flat = hist.reshape(-1)
        base = (np.arange(bh)[:, None] * w + np.arange(w)[None, :]) * size_d
        for dy in range(-radius, radius + 1):
            py0, py1 = max(y0, -dy), min(y1, h - dy)          # output rows whose sample row y + dy is in the image
            if py0 >= py1:
                continue
            for dx in range(-radius, radius + 1):
                px0, px1 = max(0, -dx), min(w, w - dx)
                if px0 >= px1:
                    continue
                kq = k[py0 + dy:py1 + dy, px0 + dx:px1 + dx]
                t = np.abs(g[py0:py1, px0:px1] - g[py0 + dy:py1 + dy, px0 + dx:px1 + dx])
                wt = ws[dx * dx + dy * dy] * wc[t]
                ok = kq >= 0
                idx = base[py0 - y0:py1 - y0, px0:px1] + kq
                flat[idx[ok]] += wt[ok]                        # one sample per pixel and offset: no repeated index
        total = hist.sum(-1)
        cum = np.cumsum(hist, axis=-1)
        kstar = np.argmax(2 * cum >= total[..., None], axis=-1)
        res = _result(disp[y0:y1], dmin, kstar, total)
        out[y0:y1] = np.where(sel[y0:y1], res, disp[y0:y1])
    return out


def brute_force(guide, disp, dmin, size_d, select=None, radius=9, spatial=None, rng=None):
    """Per-pixel loop: gather the counting samples, sort them by label, accumulate."""
    disp = np.ascontiguousarray(disp, np.float32)
    h, w = disp.shape
    if spatial is None or rng is None:
        spatial, rng = weight_tables(radius, 9.0, 25.5)
    k = labels(disp, dmin, size_d)
    sel = selected(select, dmin, disp.shape)
    out = disp.copy()
    for y in range(h):
        for x in range(w):
            if not sel[y, x]:
                continue
            samples = []
            for qy in range(max(0, y - radius), min(h, y + radius + 1)):
                for qx in range(max(0, x - radius), min(w, x + radius + 1)):
                    if k[qy, qx] < 0:
                        continue
                    t = abs(int(guide[y, x]) - int(guide[qy, qx]))
                    samples.append((int(k[qy, qx]), int(spatial[(qx - x) ** 2 + (qy - y) ** 2]) * int(rng[t])))
            total = sum(s[1] for s in samples)
            if total == 0:
                continue
            cum = 0
            for lab, wt in sorted(samples):
                cum += wt
                if 2 * cum >= total:
                    out[y, x] = np.float32(dmin + lab)
                    break
    return out
