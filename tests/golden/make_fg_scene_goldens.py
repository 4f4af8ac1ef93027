"""Fixture of the scene-instance tests (tests/test_fg_scene.py, tests/test_gpu_fg_scene.py): tests/golden/fg_scene/scenes.npz.

``example/*``: the boxes and small masks of the reference's example scene 77742204, reduced to 192 x 192 as tests/golden/bg_scene
reduces its sketch and inner mask (every 4th pixel; those two arrays are read from that fixture, not stored again).  A box
(y1, x1, y2, x2) becomes ((y1+3)//4, (x1+3)//4, y2//4, x2//4): the reduced pixels that lie inside it.  A small mask is cut from
the expanded 768 x 768 mask at [::4, ::4], rows y1'..y2' and columns x1'..x2' inclusive, as pred_masks holds them.  Data only.
Only possible where the reference's examples are at hand; run from the repo root:
    python tests/golden/make_fg_scene_goldens.py <examples directory>

``synthetic/*``: one 96 x 96 scene for the generator size 64: grass (class 27) with strokes over it, a road (36) whose mask is
two parallel bands, a house (15) whose box is exactly 64 x 64, an instance of class 40 (a class the instance generator does not
colour), a tree (43) whose box ends in the last row and column; boxes with odd and even x1; mask bytes 0, 1 and 2."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if len(sys.argv) != 2:
    sys.exit(__doc__)
EXAMPLES = sys.argv[1]
ID = '77742204'

out = {}
with np.load(os.path.join(EXAMPLES, 'seg_data', ID + '_datas.npz'), allow_pickle=True) as npz:
    ids, boxes, smalls = np.array(npz['pred_class_ids']), np.array(npz['pred_boxes'], np.int32), list(npz['pred_masks'])
bg = np.load(os.path.join(HERE, 'bg_scene', 'scenes.npz'))
assert np.array_equal(bg['example/class_ids'], ids)
new_boxes = []
for k, ((y1, x1, y2, x2), small) in enumerate(zip(boxes.tolist(), smalls)):
    full = np.zeros((768, 768), np.uint8)
    full[y1:y2 + 1, x1:x2 + 1] = small
    b = [(y1 + 3) // 4, (x1 + 3) // 4, y2 // 4, x2 // 4]
    new_boxes.append(b)
    out['example/mask_%d' % k] = np.ascontiguousarray(full[::4, ::4][b[0]:b[2] + 1, b[1]:b[3] + 1])
out['example/boxes'] = np.array(new_boxes, np.int32)
out['example/n'] = np.array(len(new_boxes))

# ---------------------------------------------------------------------------------------------------------------
H = W = 96
s_ids = np.array([27, 36, 15, 40, 43], np.int32)
s_boxes = np.array([[62, 5, 92, 51],        # grass: odd x1
                    [44, 2, 58, 94],        # road: even x1, margin 0
                    [0, 30, 64, 94],        # house: exactly 64 x 64, even x1
                    [2, 3, 22, 25],         # class 40: not coloured
                    [66, 61, 96, 96]],      # tree: odd x1, ends in the last row and column
                   np.int32)
sketch = np.full((H, W, 3), 255, np.uint8)
inner = np.zeros((H, W), np.uint8)
masks = []
rng = np.random.RandomState(41)
for k, (y1, x1, y2, x2) in enumerate(s_boxes.tolist()):
    bh, bw = y2 - y1, x2 - x1
    m = np.zeros((bh + 1, bw + 1), np.uint8)
    if s_ids[k] == 36:                      # two bands along the road, three pixels thick
        m[1:4, :bw] = 1
        m[bh - 4:bh - 1, :bw] = 1
    elif s_ids[k] == 27:                    # blades of grass
        for x in range(2, bw - 1, 5):
            m[3:bh - 2, x] = 1
        m[bh - 3, 1:bw - 1] = 1
    else:                                   # an outline and a line through the middle
        m[1, 1:bw - 1] = m[bh - 2, 1:bw - 1] = 1
        m[1:bh - 1, 1] = m[1:bh - 1, bw - 2] = 1
        m[bh // 2, 1:bw - 1] = 1
    m[0, 0] = 2                             # a byte that is neither 0 nor 1: white in the mask image
    m[bh // 2, bw // 2 + 1] = 2 if m[bh // 2, bw // 2 + 1] == 0 else m[bh // 2, bw // 2 + 1]
    m[bh, :] = 1                            # the last row and column lie outside the box: never read
    m[:, bw] = 1
    masks.append(m)
    region = np.zeros((H, W), bool)
    region[y1 + 1:y2 - 1, x1 + 1:x2 - 1] = True
    inner[region & (inner == 0)] = k + 1    # earlier instances keep their pixels where boxes overlap
    strokes = np.zeros((H, W), bool)
    strokes[y1:y2, x1:x2] = m[:bh, :bw] == 1
    sketch[strokes & (inner == k + 1)] = 0
inner[rng.rand(H, W) < 0.02] = 0
sketch[0, 40:60] = 0
sketch[30:50, 0] = 0
sketch[95, 10:40] = 0
for k, m in enumerate(masks):
    out['synthetic/mask_%d' % k] = m
out.update({'synthetic/sketch': sketch, 'synthetic/inner': inner, 'synthetic/class_ids': s_ids, 'synthetic/boxes': s_boxes,
            'synthetic/n': np.array(len(masks))})

d = os.path.join(HERE, 'fg_scene')
os.makedirs(d, exist_ok=True)
np.savez_compressed(os.path.join(d, 'scenes.npz'), **out)
print(os.path.getsize(os.path.join(d, 'scenes.npz')), 'bytes')
