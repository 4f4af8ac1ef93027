"""Full-reference image scores of the evaluation modes, the host side: the SSIM window, and the step from the five sums per
image that hip.image_metrics_u8 returns (sum |a-b|, sum (a-b)^2, counted pixels, SSIM sum, counted windows per channel) to MAE,
PSNR and SSIM per image, per group and over everything; and the step from the confusion counts of hip.seg_confusion to the region
branch's pixel accuracy and IoU.  NumPy only: nothing here needs a GPU."""
import json
import math

import numpy as np

WINDOW, SIGMA = 11, 1.5     # Wang et al. 2004: an 11 x 11 circular-symmetric Gaussian of standard deviation 1.5


def ssim_window():
    """The 11 float64 weights exp(-(i-5)^2 / (2 * 1.5^2)), normalised to sum 1: the kernel and every oracle take these."""
    i = np.arange(WINDOW, dtype=np.float64) - (WINDOW // 2)
    w = np.exp(-(i * i) / (2.0 * SIGMA * SIGMA))
    return w / w.sum()


def scores(rows):
    """[N,5] sums -> one dict per image: mae, mse, psnr (None when mse is 0: infinite, JSON null), ssim (None without a
    window).  An image without a counted pixel has no value at all."""
    out = []
    for r in np.asarray(rows, dtype=np.float64).reshape(-1, 5):
        sad, sse, pixels, ssim_sum, windows = (float(v) for v in r)
        mae = sad / (3.0 * pixels) if pixels > 0 else None
        mse = sse / (3.0 * pixels) if pixels > 0 else None
        psnr = 10.0 * math.log10(255.0 * 255.0 / mse) if mse else None
        ssim = ssim_sum / (3.0 * windows) if windows > 0 else None
        out.append({'mae': mae, 'mse': mse, 'psnr': psnr, 'ssim': ssim})
    return out


def _mean(values):
    values = [v for v in values if v is not None]
    return sum(values) / len(values) if values else None


def _group(items):
    """Means over the images that have a value; psnr over the finite ones, with the count of infinite ones beside it."""
    return {'n': len(items), 'mae': _mean([s['mae'] for s in items]), 'psnr': _mean([s['psnr'] for s in items]),
            'psnr_infinite': sum(1 for s in items if s['psnr'] is None and s['mse'] == 0.0),
            'ssim': _mean([s['ssim'] for s in items])}


def summarise(names, groups, rows):
    """names[i], groups[i]: the name and the group of image i, rows: [N,5] -> {'images': {name: {mae, psnr, ssim}},
    'groups': {group: {n, mae, psnr, psnr_infinite, ssim}}, 'all': {...}}, every level with sorted keys."""
    per = scores(rows)
    assert len(names) == len(groups) == len(per), (len(names), len(groups), len(per))
    order = sorted(range(len(per)), key=lambda i: (str(names[i]), i))       # means are summed in name order: the order the
    per, names, groups = [per[i] for i in order], [str(names[i]) for i in order], [str(groups[i]) for i in order]   # images came in does not show
    by_group = {}
    for g, s in zip(groups, per):
        by_group.setdefault(g, []).append(s)
    return {'all': _group(per), 'groups': {g: _group(by_group[g]) for g in sorted(by_group)},
            'images': {n: {'mae': s['mae'], 'psnr': s['psnr'], 'ssim': s['ssim']} for n, s in zip(names, per)}}


def dumps(summary):
    """The text of metrics.json: sorted keys, so that two runs over the same images write equal files."""
    return json.dumps(summary, indent=1, sort_keys=True) + '\n'


def all_line(summary):
    """The line the command lines print."""
    a = summary['all']
    fmt = lambda v, f: 'n/a' if v is None else f % v      # noqa: E731
    return 'metrics: n %d  mae %s  psnr %s dB (%d infinite)  ssim %s' % (
        a['n'], fmt(a['mae'], '%.4f'), fmt(a['psnr'], '%.3f'), a['psnr_infinite'], fmt(a['ssim'], '%.6f'))


def region_scores(conf):
    """Confusion counts [K*K+1] or [S, K*K+1] (hip.seg_confusion: cell t*K+p = pixels with label t and prediction p, the last
    slot = pixels whose label lies outside [0, K); samples are added) -> {'accuracy': trace / counted pixels, 'iou': [TP / (TP +
    FP + FN) per class, None for a class with TP + FP + FN == 0], 'miou': the mean over the classes that have a value,
    'ignored': the last slot}.  accuracy and miou are None when nothing is counted."""
    c = np.asarray(conf, dtype=np.int64)
    c = c.reshape(-1, c.shape[-1]).sum(0)
    k = int(round(math.sqrt(c.size - 1)))
    assert k >= 1 and k * k + 1 == c.size, c.size
    m = [[int(v) for v in row] for row in c[:k * k].reshape(k, k)]
    counted = sum(sum(row) for row in m)
    iou = []
    for j in range(k):
        tp = m[j][j]
        union = sum(m[j]) + sum(m[t][j] for t in range(k)) - tp        # TP + FN + FP
        iou.append(tp / union if union > 0 else None)
    return {'accuracy': sum(m[j][j] for j in range(k)) / counted if counted > 0 else None, 'iou': iou, 'miou': _mean(iou),
            'ignored': int(c[-1])}
