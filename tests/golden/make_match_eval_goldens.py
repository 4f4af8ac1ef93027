"""Fixtures of the matcher-evaluation tests (tests/test_match_eval.py, tests/test_gpu_match_eval.py): tests/golden/match_eval/.

Recorded from the reference's own functions, imported here and nowhere else -- data only, what they return for fixed inputs:
    metrics.npz     a crafted 40 x 40 scene (a ground-truth label map of seven instances, seven predicted instances as boxes and
                    small masks) and six captions, each a ``predicts`` image and its inst_indices.  Per caption:
                    utils/eval_tools.py::compute_mask_IU(predicts, target), data_processing/sketch_data_processing.py::
                    get_pred_instance_mask(npz, predicts) (matched indices, scores), eval_tools.compute_ap(gt masks, scores,
                    pred masks, t) for the ten thresholds of np.linspace(.5, .95, 10) stored as float32 [10] the way
                    matching_main.py stores them, and the overlaps compute_ap returns (compute_overlaps_masks of the
                    predictions in its sorted order).  Covered: overlapping predicted instances, two predictions with equal
                    scores, two ground-truth columns with equal overlap (a listed duplicate, and a prediction that is the union
                    of two equal instances: overlap exactly 0.5 with both), overlaps of exactly 0.7 and 0.6 (as float32 the first
                    lies below the float64 threshold, the second above), a caption with no prediction, mask bytes of 2 and 3.
                    Also the float32 means the reference prints (np.mean of the list of float32 vectors).
    augment.json    data_processing/text_processing.py::augment_the_caption_with_attr under random.seed(0 .. 19) for one caption
                    of every branch
Only possible where the reference is at hand; from the repository root:
    python tests/golden/make_match_eval_goldens.py <reference root>"""
import json
import os
import random
import shutil
import sys
import tempfile
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if len(sys.argv) != 2:
    sys.exit(__doc__)
REF = os.path.abspath(sys.argv[1])
sys.path.insert(0, os.path.join(REF, 'Instance_Matching'))
from data_processing import text_processing                 # noqa: E402
from data_processing import sketch_data_processing as sdp   # noqa: E402
from utils import eval_tools                                # noqa: E402

OUT = os.path.join(HERE, 'match_eval')
os.makedirs(OUT, exist_ok=True)
S = 40
THRESHOLDS = np.linspace(.5, .95, 10)


def scene():
    rng = np.random.RandomState(7)
    labels = np.zeros((S, S), np.uint8)
    labels[2:12, 2:12] = 1          # G0, 100 pixels
    labels[2:12, 20:30] = 2         # G1
    labels[20:30, 2:12] = 3         # G2
    labels[20:30, 20:30] = 4        # G3
    labels[32:38, 5:35] = 5         # G4, 180 pixels
    labels[14:18, 30:34] = 6        # G5, 16 pixels
    labels[14:18, 34:38] = 7        # G6, 16 pixels
    boxes, masks = [], []

    def add(y1, x1, y2, x2, m):
        boxes.append([y1, x1, y2, x2])
        masks.append(np.ascontiguousarray(np.broadcast_to(m, (y2 - y1 + 1, x2 - x1 + 1)), dtype=np.uint8))
    add(2, 2, 11, 11, 1)                                    # P0 = G0
    m = np.ones((10, 7), np.uint8)
    m[0, :5] = 2
    add(2, 20, 11, 26, m)                                   # P1: 70 of G1's 100 pixels, five bytes of 2: overlap 0.7
    m = np.ones((10, 6), np.uint8)
    m[9, :4] = 3
    add(20, 2, 29, 7, m)                                    # P2: 60 of G2's 100 pixels, four bytes of 3: overlap 0.6
    add(20, 7, 29, 24, 1)                                   # P3: 50 pixels of G2 and 50 of G3, overlaps P2's box
    add(14, 30, 17, 37, 1)                                  # P4 = G5 + G6: overlap 0.5 with either
    add(0, 0, 13, 13, 1)                                    # P5 holds P0: overlap 100 / 196 with G0
    m = (rng.rand(8, 32) < 0.9).astype(np.uint8)
    m[1, 3:6] *= 2
    m[6, 20:22] *= 3
    add(31, 4, 38, 35, m)                                   # P6 over G4 with holes and bytes of 2 and 3
    boxes = np.array(boxes, np.int32)

    def blank():
        return np.zeros((S, S), np.float32)
    captions = []
    p = blank()
    p[0:14, 0:14] = 1                                       # P0 and P5 with score 1 both
    p[0, 0] = 128                                           # a grey byte of the stroke map stays a non-zero value
    captions.append((p, [0]))
    p = blank()
    p[2:12, 20:27] = 1
    p[11, 20:27] = 0                                        # P1 with 63 of its 70 pixels, 63 / 75 by bytes
    p[20:30, 2:8] = 1                                       # P2 whole
    p[25, 30:36] = 1                                        # pixels outside every target
    captions.append((p, [1, 2]))
    p = blank()
    p[14:18, 30:38] = 1
    captions.append((p, [5, 6]))
    p = blank()
    p[::5, ::3] = 1                                         # thin: no instance is covered by more than a half
    captions.append((p, [3]))
    captions.append((captions[0][0].copy(), [0, 0]))        # a duplicate in the list: two equal columns
    p = (rng.rand(S, S) < 0.6).astype(np.float32)
    p[31:39, 4:36] = (rng.rand(8, 32) < 0.9)
    p[5, 5] = 2
    captions.append((p, [3, 4, 2]))
    return labels, boxes, masks, captions


labels, boxes, masks, captions = scene()
sdp.IMAGE_SIZE = S
out = {'labels': labels, 'boxes': boxes, 'n': np.array(len(masks)), 'n_captions': np.array(len(captions)), 'thresholds': THRESHOLDS}
for k, m in enumerate(masks):
    out['mask_%d' % k] = m
tmp = tempfile.mkdtemp()
aps = []
try:
    path = os.path.join(tmp, 'scene_datas.npz')
    obj = np.empty(len(masks), dtype=object)
    for k, m in enumerate(masks):
        obj[k] = m
    np.savez(path, pred_masks=obj, pred_boxes=boxes, pred_class_ids=np.arange(len(masks), dtype=np.int32) + 1)
    _load = np.load
    np.load = lambda p, **kw: _load(p, allow_pickle=True)       # the reference predates numpy's allow_pickle default
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            for c, (predicts, inst) in enumerate(captions):
                gt = np.zeros((S, S, len(inst)), np.int32)
                target = np.zeros((S, S), np.int32)
                for t, i in enumerate(inst):
                    target = np.logical_or(target, labels == i + 1)
                    gt[:, :, t] = labels == i + 1
                I, U = eval_tools.compute_mask_IU(predicts.copy(), target)
                pred_masks, scores, _, _, matched = sdp.get_pred_instance_mask(path, predicts.copy())
                ap = np.zeros(len(THRESHOLDS), np.float32)
                ov = np.zeros((0, len(inst)), np.float32)
                if scores.shape[0] != 0:
                    for j, t in enumerate(THRESHOLDS):
                        ap[j], _, _, ov = eval_tools.compute_ap(gt, scores, pred_masks, iou_threshold=t)
                    assert ov.dtype == np.float32
                aps.append(ap)
                tag = 'c%d/' % c
                out[tag + 'predicts'] = predicts.astype(np.uint8)
                assert np.array_equal(out[tag + 'predicts'] != 0, predicts != 0)
                out[tag + 'inst_indices'] = np.array(inst, np.int64)
                out[tag + 'I'], out[tag + 'U'] = np.array(int(I)), np.array(int(U))
                out[tag + 'matched'] = np.array(matched, np.int64)
                out[tag + 'scores'] = np.array(scores, np.float64).reshape(-1)
                out[tag + 'overlaps'] = ov
                out[tag + 'ap'] = ap
                print(c, inst, 'I', I, 'U', U, 'matched', matched, 'scores', scores, 'ap', ap)
    finally:
        np.load = _load
finally:
    shutil.rmtree(tmp)
out['mAP'] = np.array(np.mean(aps))
out['mAP_list'] = np.mean(aps, axis=0)
assert out['mAP_list'].dtype == np.float32
np.savez_compressed(os.path.join(OUT, 'metrics.npz'), **out)

CAPTIONS = ['the person on the left', 'the bus in the middle', 'the house on the right of the tree', 'the bird', 'the car',
            'the butterfly near the tree', 'the dog on the left', 'the sheep', 'two trees on the right', 'all the people',
            'the butterflies', 'the left-most cloud']
aug = {}
for c in CAPTIONS:
    aug[c] = []
    for seed in range(20):
        random.seed(seed)
        aug[c].append(text_processing.augment_the_caption_with_attr(c))
with open(os.path.join(OUT, 'augment.json'), 'w') as f:
    json.dump(aug, f, indent=1)
print(sum(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT)), 'bytes')
