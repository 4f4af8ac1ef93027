"""Float64 NumPy oracle of ssc_image_metrics_u8 (helper, not a test module): the five sums per image, by the definitions of
include/sketchycolor_hip.h, written twice -- a separable "valid" pass and a direct loop over windows with the full 11 x 11
outer-product weights -- so that the oracle checks itself before it checks the kernel."""
import numpy as np

C1 = (0.01 * 255) ** 2
C2 = (0.03 * 255) ** 2


def _ssim_from_moments(mx, my, mxx, myy, mxy):
    vx, vy, cov = mxx - mx * mx, myy - my * my, mxy - mx * my
    return ((2 * mx * my + C1) * (2 * cov + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2))


def _valid_1d(x, win, axis):
    """'valid' correlation of x with the 11 weights along ``axis``."""
    n = x.shape[axis] - len(win) + 1
    out = np.zeros(x.shape[:axis] + (n,) + x.shape[axis + 1:], np.float64)
    for k, w in enumerate(win):
        out += w * np.take(x, np.arange(k, k + n), axis=axis)
    return out


def ssim_map_separable(a, b, win):
    """a, b uint8 [H,W,3] -> the SSIM of every valid window, float64 [H-10, W-10, 3] (rows first, then columns)."""
    x, y = a.astype(np.float64), b.astype(np.float64)
    f = lambda t: _valid_1d(_valid_1d(t, win, 0), win, 1)      # noqa: E731
    return _ssim_from_moments(f(x), f(y), f(x * x), f(y * y), f(x * y))


def ssim_map_direct(a, b, win):
    """The same map from one 121-term weighted sum per window, moment and channel."""
    h, w, _ = a.shape
    x, y = a.astype(np.float64), b.astype(np.float64)
    w2 = np.outer(win, win)[:, :, None]
    k = len(win)
    out = np.zeros((h - k + 1, w - k + 1, 3), np.float64)
    for i in range(h - k + 1):
        for j in range(w - k + 1):
            px, py = x[i:i + k, j:j + k], y[i:i + k, j:j + k]
            m = [(w2 * t).sum(axis=(0, 1)) for t in (px, py, px * px, py * py, px * py)]
            out[i, j] = _ssim_from_moments(*m)
    return out


def rows(a, b, win, mask=None, ssim_map=ssim_map_separable):
    """a, b uint8 [N,H,W,3], mask uint8 [N,H,W] or None -> float64 [N,5]: sum |a-b|, sum (a-b)^2, counted pixels, SSIM sum over
    the counted windows (centre pixel counted) and the 3 channels, counted windows per channel."""
    n, h, w, _ = a.shape
    out = np.zeros((n, 5), np.float64)
    for i in range(n):
        keep = np.ones((h, w), bool) if mask is None else mask[i] != 0
        d = a[i].astype(np.int64) - b[i].astype(np.int64)
        out[i, 0] = np.abs(d)[keep].sum()
        out[i, 1] = (d * d)[keep].sum()
        out[i, 2] = keep.sum()
        if h >= 11 and w >= 11:
            centre = keep[5:h - 5, 5:w - 5]
            out[i, 3] = ssim_map(a[i], b[i], win)[centre].sum()
            out[i, 4] = centre.sum()
    return out
