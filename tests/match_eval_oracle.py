"""The matcher's evaluation restated on full-size masks in NumPy, for tests/test_match_eval.py and tests/test_gpu_match_eval.py:
what Instance_Matching/matching_main.py --mode eval computes per caption, from images instead of
histograms.  Counts are integers, scores and thresholds float64, overlaps and stored APs float32 as in the reference."""
import json
import os

import numpy as np

THRESHOLDS = np.linspace(.5, .95, 10)
LEVELS = (.5, .6, .7, .8, .9)


def expand(boxes, masks, size):
    """The small masks laid at their boxes: uint8 [N, size, size], the bytes kept."""
    out = np.zeros((len(masks), size, size), np.uint8)
    for k, ((y1, x1, y2, x2), m) in enumerate(zip(np.asarray(boxes).tolist(), masks)):
        out[k, y1:y2 + 1, x1:x2 + 1] = m
    return out


def target_of(labels, inst_indices):
    t = np.zeros(labels.shape, bool)
    for i in inst_indices:
        t |= labels == i + 1
    return t


def mask_iu(predicts, target):
    p, t = predicts != 0, target != 0
    return int((p & t).sum()), int((p | t).sum())


def select(predicts, full):
    """-> (matched indices, float64 occupancy of each of them): pixels where both are non-zero over the sum of the mask's bytes,
    matched above 0.5."""
    matched, scores = [], []
    for k in range(len(full)):
        inter, total = int(((predicts != 0) & (full[k] != 0)).sum()), int(full[k].astype(np.int64).sum())
        if total > 0 and inter / total > 0.5:
            matched.append(k)
            scores.append(inter / total)
    return matched, np.array(scores, np.float64)


def overlaps(pred_full, gt_full):
    """float32 [n, m]: intersection over union of every pair, the counts turned to float32 before the sum and the quotient."""
    out = np.zeros((len(pred_full), len(gt_full)), np.float32)
    for i, p in enumerate(pred_full):
        for j, g in enumerate(gt_full):
            inter = np.float32(int(((p != 0) & (g != 0)).sum()))
            a, b = np.float32(int((p != 0).sum())), np.float32(int((g != 0).sum()))
            out[i, j] = inter / (a + b - inter)
    return out


def _descending(v):
    """Indices by descending value; of equal values the one with the larger index first."""
    return sorted(range(len(v)), key=lambda i: (v[i], i), reverse=True)


def average_precision(scores, ov, threshold):
    """ov in the order of scores.  Greedy matching in descending score, each prediction to its best free ground-truth column
    unless the overlap is below the threshold; AP as the area under the precision envelope over the float32 recall steps."""
    order = _descending(list(scores))
    n, m = len(order), ov.shape[1]
    taken, hit = [False] * m, []
    for i in order:
        ok = 0
        for j in _descending(list(ov[i])):
            if taken[j]:
                continue
            if float(ov[i, j]) >= float(threshold):
                taken[j], ok = True, 1
            break
        hit.append(ok)
    tp = np.cumsum(hit).astype(np.float64)
    prec = [0.0] + [tp[k] / (k + 1) for k in range(n)] + [0.0]
    rec = [0.0] + [float(np.float32(tp[k]) / np.float32(m)) for k in range(n)] + [1.0]
    for k in range(len(prec) - 2, -1, -1):
        prec[k] = max(prec[k], prec[k + 1])
    return sum((rec[k] - rec[k - 1]) * prec[k] for k in range(1, len(rec)) if rec[k] != rec[k - 1])


def caption(predicts, labels, full, inst_indices):
    """-> {I, U, matched, scores, ap float32 [10]} of one caption."""
    I, U = mask_iu(predicts, target_of(labels, inst_indices))
    matched, scores = select(predicts, full)
    ap = np.zeros(len(THRESHOLDS), np.float32)
    if matched:
        ov = overlaps(full[matched], [labels == i + 1 for i in inst_indices])
        for j, t in enumerate(THRESHOLDS):
            ap[j] = average_precision(scores, ov, t)
    return {'I': I, 'U': U, 'matched': matched, 'scores': scores, 'ap': ap}


def totals(results):
    """-> {cum_I, cum_U, overall_IoU, precision [5], mAP, mAP_list [10]} of a list of ``caption`` results."""
    cum_I, cum_U = sum(r['I'] for r in results), sum(r['U'] for r in results)
    aps = np.array([r['ap'] for r in results], np.float64)
    return {'cum_I': cum_I, 'cum_U': cum_U, 'overall_IoU': cum_I / cum_U,
            'precision': [sum(int(r['I'] / r['U'] >= t) for r in results) / float(len(results)) for t in LEVELS],
            'mAP': float(aps.mean()), 'mAP_list': aps.mean(axis=0)}


def block(snapshot, tot, mask_ap=True):
    s = '\n' + snapshot + '\nSegmentation evaluation (without DenseCRF):\n'
    for t, p in zip(LEVELS, tot['precision']):
        s += 'precision@%s = %f\n' % (str(t), p)
    s += 'overall IoU = %f\n' % tot['overall_IoU']
    if mask_ap:
        s += 'iou_threshold @[0.5:0.95],  mAP = %s\n' % str(np.float64(tot['mAP']))
        s += 'mAP_list = %s\n' % str(tot['mAP_list'])
    return s


def write_split(base, split='val', size_gt=60, size=64, scenes=('11', '12'), seed=0):
    """A synthetic split under ``base``: data/<split>/{INSTANCE_GT, DRAWING_GT}, captions/sentence_instance_<split>.json,
    seg/<split>/seg_data.  -> the flags that point at it."""
    import scipy.io
    from PIL import Image
    rng = np.random.RandomState(seed)
    data, caps, seg = os.path.join(base, 'data'), os.path.join(base, 'captions'), os.path.join(base, 'seg')
    for d in (os.path.join(data, split, 'INSTANCE_GT'), os.path.join(data, split, 'DRAWING_GT'), caps, os.path.join(seg, split, 'seg_data')):
        os.makedirs(d, exist_ok=True)
    entries = []
    for key in scenes:
        gt = np.zeros((size_gt, size_gt), np.uint8)
        rects = [(2, 2, 20, 24), (4, 30, 26, 56), (30, 4, 56, 28), (34, 32, 50, 58), (52, 40, 58, 58)]
        for k, (y1, x1, y2, x2) in enumerate(rects):
            gt[y1:y2, x1:x2] = (k + 1) * 5             # gaps in the ids
        scipy.io.savemat(os.path.join(data, split, 'INSTANCE_GT', 'sample_%s_instance.mat' % key), {'INSTANCE_GT': gt})
        sk = np.full((size, size, 3), 255, np.uint8)
        sk[rng.rand(size, size) < 0.5] = 0
        Image.fromarray(sk).save(os.path.join(data, split, 'DRAWING_GT', 'L0_sample%s.png' % key))
        boxes, masks = [], []
        for (y1, x1, y2, x2) in rects + [(0, 0, 30, 30), (28, 28, 62, 62)]:
            b = [y1 + int(rng.randint(0, 3)), x1 + int(rng.randint(0, 3)), min(size - 1, y2 + int(rng.randint(0, 4))),
                 min(size - 1, x2 + int(rng.randint(0, 4)))]
            m = (rng.rand(b[2] - b[0] + 1, b[3] - b[1] + 1) < 0.9).astype(np.uint8)
            m[0, 0] = 2
            boxes.append(b)
            masks.append(m)
        obj = np.empty(len(masks), dtype=object)
        for k, m in enumerate(masks):
            obj[k] = m
        np.savez(os.path.join(seg, split, 'seg_data', '%s_datas.npz' % key), pred_masks=obj, pred_boxes=np.array(boxes, np.int32),
                 pred_class_ids=np.arange(len(masks)) + 3)
        entries.append({'key': int(key), 'sen_instIdx_map': {'the house on the left': [0], 'two trees on the right': [1, 3],
                                                             'all the people near the bus': [2, 4, 2]}})
    with open(os.path.join(caps, 'sentence_instance_%s.json' % split), 'w') as f:
        json.dump(entries, f)
    return ['--data_base_dir', data, '--captions_base_dir', caps, '--seg_data_dir', seg, '--dataset', split]
