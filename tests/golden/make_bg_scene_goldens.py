"""Fixture of the scene-background tests (tests/test_bg_scene.py, tests/test_gpu_bg_scene.py): tests/golden/bg_scene/scenes.npz.

``example/*``: the reference's example scene 77742204 -- the sketch as the pipeline loads it (RGB, nearest-neighbour to 768 x
768), its inner mask and pred_class_ids ([36 43 43 43 43 43 43 15 32]: no grass) -- reduced to 192 x 192 by taking every 4th
pixel.  Data only; the 768 x 768 .mat is not stored.  Only possible where the reference's examples are at hand; run from the
repo root:  python tests/golden/make_bg_scene_goldens.py [examples directory]

``grass/*``: a synthetic 192 x 192 scene in which instance 1 (mask value 2) has class 27, with strokes over it, over a
non-grass instance, in row 0, in column 0 and in the last row and column."""
import os
import sys

import numpy as np
import scipy.io
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
EXAMPLES = sys.argv[1] if len(sys.argv) > 1 else '/root/reference/examples'
ID = '77742204'

sketch = Image.open(os.path.join(EXAMPLES, 'sketches', ID + '.png')).convert('RGB').resize((768, 768), resample=Image.NEAREST)
sketch = np.array(sketch, dtype=np.uint8)[::4, ::4]
inner = scipy.io.loadmat(os.path.join(EXAMPLES, 'inner_masks', ID + '.mat'))['inner_masks'][::4, ::4]
ids = np.load(os.path.join(EXAMPLES, 'seg_data', ID + '_datas.npz'))['pred_class_ids']
assert sketch.shape == (192, 192, 3) and inner.shape == (192, 192) and inner.dtype == np.uint8 and 27 not in ids

rng = np.random.RandomState(27)
g_inner = np.zeros((192, 192), np.uint8)
g_inner[100:150, 20:90] = 1         # instance 0: a house (class 15)
g_inner[140:192, 80:192] = 2        # instance 1: grass (class 27), down to the last row and column
g_inner[30:60, 120:160] = 3         # instance 2: a cloud (class 10) in the upper half
g_sketch = np.full((192, 192, 3), 255, np.uint8)
for _ in range(60):                 # short black strokes all over, some grey ones (red byte not 0: not drawn)
    y, x = rng.randint(0, 192, 2)
    n = rng.randint(3, 30)
    colour = 0 if rng.rand() < 0.8 else 120
    if rng.rand() < 0.5:
        g_sketch[y, x:x + n] = colour
    else:
        g_sketch[y:y + n, x] = colour
g_sketch[0, 10:40] = 0
g_sketch[50:90, 0] = 0
g_sketch[191, 150:192] = 0
g_sketch[160:192, 191] = 0
g_ids = np.array([15, 27, 10], np.int32)

d = os.path.join(HERE, 'bg_scene')
os.makedirs(d, exist_ok=True)
np.savez_compressed(os.path.join(d, 'scenes.npz'), **{
    'example/sketch': sketch, 'example/inner': inner, 'example/class_ids': ids,
    'grass/sketch': g_sketch, 'grass/inner': g_inner, 'grass/class_ids': g_ids})
print(os.path.getsize(os.path.join(d, 'scenes.npz')), 'bytes')
