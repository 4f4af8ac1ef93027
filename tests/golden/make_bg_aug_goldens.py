"""The fixture tests/golden/bg_aug/: two tiny scenes and everything the REFERENCE's own dataset generator
(Background_Colorization/data_preparation/bg_data_generation.py, numpy + PIL only) writes for them with aug_num = 3 -- the base
and augmented backgrounds, the segment maps and captions/train.json -- plus a copy of its 18-word vocabulary list.  Only possible
where the reference is at hand (it does not travel); run from the repo root:

    python tests/golden/make_bg_aug_goldens.py /path/to/the/reference

The scenes (16 x 16 and 12 rows x 20 columns) have a blue top row and a green bottom row (the generator asserts that), a foreground
patch (inner_mask 0) one of whose pixels is exactly the sky blue, background pixels that are neither blue nor green (a dark
separating line, a few strays) and a blue pixel under an inner_mask value that is neither 0 nor 255."""
import importlib.util
import os
import random
import shutil
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1]
spec = importlib.util.spec_from_file_location('ref_bg_data_generation',
                                              os.path.join(REF, 'Background_Colorization', 'data_preparation', 'bg_data_generation.py'))
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)

out = os.path.join(HERE, 'bg_aug')
if os.path.exists(out):
    shutil.rmtree(out)
for kind in ('user_paint', 'foreground', 'inner_mask'):
    for split in ('train', 'test'):
        os.makedirs(os.path.join(out, kind, split))

BLUE, GREEN = ref.color_map['blue'], ref.color_map['green']
rng = np.random.RandomState(20261017)
for name, (H, W) in (('scene_a.png', (16, 16)), ('scene_b.png', (12, 20))):
    paint = np.zeros((H, W, 3), np.uint8)
    horizon = H // 2 + 1
    paint[:horizon] = BLUE
    paint[horizon:] = GREEN
    paint[horizon - 1, :] = (40, 40, 40)                    # the user's separating line: background, neither blue nor green
    for _ in range(5):                                      # strays, kept off the top and bottom rows
        paint[rng.randint(1, H - 1), rng.randint(0, W)] = rng.randint(0, 256, 3)
    mask = np.full((H, W), 255, np.uint8)
    y0, x0 = H // 4, W // 4
    mask[y0:y0 + H // 2, x0:x0 + W // 3] = 0                # the foreground patch, across the line
    fg = np.full((H, W, 3), 255, np.uint8)
    fg[mask == 0] = rng.randint(0, 256, (int((mask == 0).sum()), 3))
    fg[y0, x0] = BLUE                                       # a foreground pixel of exactly the sky colour
    fg[y0 + 1, x0] = GREEN
    mask[1, W - 2] = 100                                    # blue, but not background by the mask
    Image.fromarray(paint, 'RGB').save(os.path.join(out, 'user_paint', 'train', name))
    Image.fromarray(fg, 'RGB').save(os.path.join(out, 'foreground', 'train', name))
    Image.fromarray(np.repeat(mask[:, :, None], 3, 2), 'RGB').save(os.path.join(out, 'inner_mask', 'train', name))

random.seed(20261017)
ref.bg_data_generation(data_base_dir=out, aug_num=3)
shutil.copyfile(os.path.join(REF, 'Background_Colorization', 'data', 'bg_vocab.txt'), os.path.join(out, 'bg_vocab.txt'))
for base, dirs, files in os.walk(out, topdown=False):       # the empty test split leaves nothing to commit but its caption list
    if not dirs and not files:
        os.rmdir(base)
print(sorted(os.path.relpath(os.path.join(b, f), out) for b, _, fs in os.walk(out) for f in fs))
