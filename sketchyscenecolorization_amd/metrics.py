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


COLOR_KEYS = ('de76', 'dab', 'dl', 'hist_intersection', 'colourfulness', 'colourfulness_target')


def lab_lin_table():
    """The 256 float64 values of sRGB -> linear for a byte: c = byte / 255, c / 12.92 where c <= 0.04045, else
    ((c + 0.055) / 1.055) ** 2.4.  hip.color_metrics_* hand it to the kernel, which therefore evaluates no pow."""
    c = np.arange(256, dtype=np.float64) / 255.0
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)


def _colourfulness(n, s_rg, s_rg2, s_yb2, s_yb22):
    """Hasler & Suesstrunk 2003 from the integer sums over n pixels: rg = R - G, yb = (R + G) / 2 - B = yb2 / 2;
    sqrt(var rg + var yb) + 0.3 sqrt(mean rg ^ 2 + mean yb ^ 2), population variances."""
    m_rg, m_yb = s_rg / n, s_yb2 / (2.0 * n)
    v_rg, v_yb = s_rg2 / n - m_rg * m_rg, s_yb22 / (4.0 * n) - m_yb * m_yb
    return math.sqrt(max(v_rg + v_yb, 0.0)) + 0.3 * math.sqrt(m_rg * m_rg + m_yb * m_yb)


def color_scores(rows):
    """[N,13] sums (hip.color_metrics_u8) -> one dict per image: de76, dab, dl (means over the counted pixels), hist_intersection
    (sum min / counted pixels), colourfulness (of the output, image a) and colourfulness_target (image b).  Every score of an
    image without a counted pixel is None."""
    out = []
    for r in np.asarray(rows, dtype=np.float64).reshape(-1, 13):
        r = [float(v) for v in r]
        n = r[3]
        if n <= 0:
            out.append({k: None for k in COLOR_KEYS})
            continue
        out.append({'de76': r[0] / n, 'dab': r[1] / n, 'dl': r[2] / n, 'hist_intersection': r[12] / n,
                    'colourfulness': _colourfulness(n, *r[4:8]), 'colourfulness_target': _colourfulness(n, *r[8:12])})
    return out


def _color_group(items):
    g = {k: _mean([s[k] for s in items]) for k in COLOR_KEYS}
    g['n'] = len(items)
    return g


def summarise_color(names, groups, rows):
    """names[i], groups[i] and rows [N,13] as ``summarise`` takes them -> {'images': {name: the six scores}, 'groups': {group:
    their means over the images that have a value, and n}, 'all': {...}}; means are summed in name order."""
    per = color_scores(rows)
    assert len(names) == len(groups) == len(per), (len(names), len(groups), len(per))
    order = sorted(range(len(per)), key=lambda i: (str(names[i]), i))
    per, names, groups = [per[i] for i in order], [str(names[i]) for i in order], [str(groups[i]) for i in order]
    by_group = {}
    for g, s in zip(groups, per):
        by_group.setdefault(g, []).append(s)
    return {'all': _color_group(per), 'groups': {g: _color_group(by_group[g]) for g in sorted(by_group)},
            'images': {n: dict(s) for n, s in zip(names, per)}}


def color_line(summary):
    """The line the command lines print beside ``all_line``."""
    a = summary['all']
    fmt = lambda v, f: 'n/a' if v is None else f % v      # noqa: E731
    return 'colour: n %d  dE76 %s  dab %s  dL %s  ab-hist %s  colourfulness %s (target %s)' % (
        a['n'], fmt(a['de76'], '%.4f'), fmt(a['dab'], '%.4f'), fmt(a['dl'], '%.4f'), fmt(a['hist_intersection'], '%.6f'),
        fmt(a['colourfulness'], '%.3f'), fmt(a['colourfulness_target'], '%.3f'))


def checked_color_flag(flag, metrics, val_freq, mode, scored_modes=('test',), name='--color_metrics', metrics_flag='--metrics',
                       freq_flag='--val_freq'):
    """The value of --color_metrics: ValueError -- before anything is built -- where the run has nothing it could score: an
    evaluation mode without --metrics 1, --mode train without held-out passes, a mode that has no target."""
    if not flag:
        return 0
    if mode in scored_modes:
        if not metrics:
            raise ValueError('%s 1 scores the images that %s 1 scores: --mode %s needs %s 1 beside it'
                             % (name, metrics_flag, mode, metrics_flag))
    elif mode == 'train':
        if not val_freq or val_freq <= 0:
            raise ValueError('%s 1 scores the held-out passes: --mode train needs %s F > 0 beside it' % (name, freq_flag))
    else:
        raise ValueError('%s 1 needs a target to score against (%s 1 in an evaluation mode, %s F in --mode train), this is '
                         '--mode %s' % (name, metrics_flag, freq_flag, mode))
    return 1


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
