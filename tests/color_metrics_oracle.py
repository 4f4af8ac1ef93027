"""Float64 NumPy oracle of the colour scores (helper, not a test module), written from the formulas of DESIGN.md section 8.17 and
not from the kernel: sRGB bytes -> CIELAB, the per-pixel errors, the 23 x 23 ab histogram, the integer sums of colourfulness, the
thirteen numbers per image of hip.color_metrics_u8, and colourfulness itself from the pixels (not from the sums)."""
import numpy as np

M = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]], np.float64)
WHITE = np.array([0.95047, 1.0, 1.08883], np.float64)
DELTA = 6.0 / 29.0
BINS, WIDTH, SHIFT = 23, 10.0, 115.0


def linear(byte):
    c = np.asarray(byte, np.float64) / 255.0
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)


def f(t):
    t = np.asarray(t, np.float64)
    return np.where(t > DELTA ** 3, np.cbrt(t), t / (3.0 * DELTA ** 2) + 4.0 / 29.0)


def lab(rgb_u8):
    """uint8 [...,3] -> float64 [...,3]: L, a*, b*."""
    lin = linear(rgb_u8)
    xyz = np.stack([(lin * M[k]).sum(-1) for k in range(3)], -1) / WHITE
    fx, fy, fz = f(xyz[..., 0]), f(xyz[..., 1]), f(xyz[..., 2])
    return np.stack([116.0 * fy - 16.0, 500.0 * (fx - fy), 200.0 * (fy - fz)], -1)


def cell_unclamped(v):
    return np.floor((np.asarray(v, np.float64) + SHIFT) / WIDTH).astype(np.int64)


def cell(v):
    return np.clip(cell_unclamped(v), 0, BINS - 1)


def boundary_distance(v):
    """How far a coordinate is from the nearest cell boundary (-115, -105, ..., 115)."""
    t = (np.asarray(v, np.float64) + SHIFT) / WIDTH
    return np.abs(t - np.round(t)) * WIDTH


def histogram(lab_pixels):
    """float64 [P,3] -> int64 [529]: cell(a*) * 23 + cell(b*)."""
    idx = cell(lab_pixels[:, 1]) * BINS + cell(lab_pixels[:, 2])
    return np.bincount(idx, minlength=BINS * BINS).astype(np.int64)


def opponent_sums(rgb_u8):
    """uint8 [P,3] -> the four integers sum rg, sum rg^2, sum yb2, sum yb2^2 with rg = R - G, yb2 = R + G - 2 B."""
    p = rgb_u8.astype(np.int64)
    rg, yb2 = p[:, 0] - p[:, 1], p[:, 0] + p[:, 1] - 2 * p[:, 2]
    return [int(rg.sum()), int((rg * rg).sum()), int(yb2.sum()), int((yb2 * yb2).sum())]


def colourfulness(rgb_u8):
    """Hasler & Suesstrunk 2003 from the pixels: uint8 [P,3] -> float."""
    p = rgb_u8.astype(np.float64)
    rg, yb = p[:, 0] - p[:, 1], (p[:, 0] + p[:, 1]) / 2.0 - p[:, 2]
    return float(np.sqrt(rg.var() + yb.var()) + 0.3 * np.sqrt(rg.mean() ** 2 + yb.mean() ** 2))


def rows(a, b, mask=None):
    """a, b uint8 [N,H,W,3], mask uint8 [N,H,W] or None -> (float64 [N,13], int64 [N,2,529]).  The float sums are math.fsum's:
    the exactly rounded sum of the per-pixel values."""
    import math
    n = a.shape[0]
    out, hist = np.zeros((n, 13), np.float64), np.zeros((n, 2, BINS * BINS), np.int64)
    for i in range(n):
        keep = np.ones(a.shape[1:3], bool) if mask is None else mask[i] != 0
        pa, pb = a[i][keep], b[i][keep]
        la, lb = lab(pa), lab(pb)
        d = la - lb
        out[i, 0] = math.fsum(np.sqrt((d * d).sum(-1)))
        out[i, 1] = math.fsum(np.sqrt(d[:, 1] ** 2 + d[:, 2] ** 2))
        out[i, 2] = math.fsum(np.abs(d[:, 0]))
        out[i, 3] = keep.sum()
        out[i, 4:8] = opponent_sums(pa)
        out[i, 8:12] = opponent_sums(pb)
        hist[i, 0], hist[i, 1] = histogram(la), histogram(lb)
        out[i, 12] = np.minimum(hist[i, 0], hist[i, 1]).sum()
    return out, hist


def scores(a, b, mask=None):
    """The six scores per image straight from the pixels (a list of dicts; None where nothing is counted)."""
    res = []
    r, _ = rows(a, b, mask)
    for i in range(a.shape[0]):
        keep = np.ones(a.shape[1:3], bool) if mask is None else mask[i] != 0
        n = int(keep.sum())
        if n == 0:
            res.append(dict.fromkeys(('de76', 'dab', 'dl', 'hist_intersection', 'colourfulness', 'colourfulness_target')))
            continue
        res.append({'de76': r[i, 0] / n, 'dab': r[i, 1] / n, 'dl': r[i, 2] / n, 'hist_intersection': r[i, 12] / n,
                    'colourfulness': colourfulness(a[i][keep]), 'colourfulness_target': colourfulness(b[i][keep])})
    return res
