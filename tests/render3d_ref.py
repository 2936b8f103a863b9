"""float64 restatement of the picture the 3D env's render() is defined to be: numpy, a loop over
samples vectorised over pixels, no code shared with the product and no early exit."""
import numpy as np


def rays(view_from, box, width, height):
    """origins (H, W, 3) on the image plane through the box centre, direction d, entry / exit t0, t1 and the hit mask"""
    d = -np.asarray(view_from, float) / np.linalg.norm(view_from)
    up = np.array([0.0, 0.0, 1.0]) if abs(d[2]) <= 0.999 else np.array([0.0, 1.0, 0.0])
    right = np.cross(d, up) / np.linalg.norm(np.cross(d, up))
    upv = np.cross(right, d)
    s = np.linalg.norm(box) / min(width, height)
    px, py = np.meshgrid(np.arange(width), np.arange(height))
    p = box / 2 + s * (px + 0.5 - width / 2)[..., None] * right + s * (height / 2 - py - 0.5)[..., None] * upv
    t0, t1, hit = np.full(px.shape, -np.inf), np.full(px.shape, np.inf), np.ones(px.shape, bool)
    for a in range(3):
        if d[a] == 0:
            hit &= (p[..., a] >= 0) & (p[..., a] <= box[a])
        else:
            ta, tb = (0 - p[..., a]) / d[a], (box[a] - p[..., a]) / d[a]
            t0, t1 = np.maximum(t0, np.minimum(ta, tb)), np.minimum(t1, np.maximum(ta, tb))
    return p, d, t0, t1, hit & (t1 > t0)


def render(T, domain, size=(800, 608), view_from=(1, 1, 1), clim=(1, 2), lut=None, step=None, unit=None, bg=(1, 1, 1)):
    """T: the solver's temperature (nz, ny, nx) float64; domain (lz, ly, lx) -> uint8 (height, width, 3)"""
    V = np.flip(np.asarray(T, float), axis=1)                      # rbc3D.py:275
    n = np.array(V.shape[::-1])                                     # nx, ny, nz
    h = np.array(domain[::-1], float) / n
    box = (n - 1) * h
    step = h.min() / 2 if step is None else step
    unit = np.linalg.norm(box) / (n.mean() - 1) if unit is None else unit
    width, height = size
    p, d, t0, t1, hit = rays(view_from, box, width, height)
    length = np.where(hit, t1 - t0, 0.0)
    nfull = np.floor(length / step).astype(int)
    rest = length - nfull * step
    C, A = np.zeros(p.shape), np.zeros(p.shape[:2])
    for k in range(nfull.max() + 1):
        full = k < nfull
        active = hit & (full | ((k == nfull) & (rest > 0)))
        tau, seg = np.where(full, (k + 0.5) * step, nfull * step + rest / 2), np.where(full, step, rest)
        g = (p + np.where(active, t0 + tau, 0.0)[..., None] * d) / h
        g = np.clip(g, 0, n - 1)
        i = np.minimum(np.floor(g).astype(int), n - 2)
        f = g - i
        v = 0.0
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    w = (f[..., 0] if dx else 1 - f[..., 0]) * (f[..., 1] if dy else 1 - f[..., 1]) * (f[..., 2] if dz else 1 - f[..., 2])
                    v = v + w * V[i[..., 2] + dz, i[..., 1] + dy, i[..., 0] + dx]
        x = 255 * np.clip((np.nan_to_num(v) - clim[0]) / (clim[1] - clim[0]), 0, 1)
        m = np.minimum(np.floor(x).astype(int), 254)
        rgba = lut[m] * (1 - (x - m))[..., None] + lut[m + 1] * (x - m)[..., None]
        alpha = np.where(active & ~np.isnan(v), 1 - (1 - rgba[..., 3]) ** (seg / unit), 0.0)
        C += ((1 - A) * alpha)[..., None] * rgba[..., :3]
        A += (1 - A) * alpha
    return np.clip(np.floor(255 * (C + (1 - A)[..., None] * np.asarray(bg, float)) + 0.5), 0, 255).astype(np.uint8)
