"""Fixtures of the instance-matcher tests (tests/test_matching.py, tests/test_gpu_matching.py): tests/golden/match/.

Recorded from the reference's own functions, imported here and nowhere else -- data only, what they return for fixed inputs:
    vocab.txt        the matcher's word list (Instance_Matching/data/vocab.txt), copied
    text.json        data_processing/text_processing.py::preprocess_sentence(sentence, vocab, 15) for the sentences below
    spatial.npz      utils/processing_tools.py::generate_spatial_batch(1, h, w)[0] for (8, 8) and (12, 12)
    selection.npz    data_processing/sketch_data_processing.py::get_pred_instance_mask on synthetic 64 x 64 and 96 x 96 scenes
                     written to a temporary npz, with random ``predicts``: the matched indices, and every instance's
                     compute_mask_occupied_percentage
Only possible where the reference is at hand (NumPy, SciPy, PIL and matplotlib are what these modules import); from the
repository root:
    python tests/golden/make_match_goldens.py <reference root>"""
import json
import os
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
from utils.processing_tools import generate_spatial_batch   # noqa: E402

OUT = os.path.join(HERE, 'match')
os.makedirs(OUT, exist_ok=True)
shutil.copyfile(os.path.join(REF, 'Instance_Matching', 'data', 'vocab.txt'), os.path.join(OUT, 'vocab.txt'))
vocab = text_processing.load_vocab_dict_from_file(os.path.join(OUT, 'vocab.txt'))

SENTENCES = [
    'the bus on the left is yellow',
    'The Bus On The Left Is Yellow.',
    'the tree on the right-most side is dark green',
    'the left - most cloud',
    'all the trees are light green',
    'the second person from the left is in blue shirt and red pants',
    'the zeppelin behind the xylophone',                                          # unknown words
    'the house in the middle has red roof with yellow windows .',
    'the two sheep on the right of the road , near the big tree , are light gray and dark brown',   # longer than 15
    'sun',
    '  the   moon is   yellow  ',
    "the dog's tail",
    'the car, the bus and the truck',
    'the bird at the top-left corner is red with blue wings.',
    'the 2 chickens',
    'grass!',
    'the cow under the tree is dark brown. ',
    'THE ROAD IS DARK GRAY',
    'the star -- the small one',
    'the duck on the left of the bench is orange',
    'a b c d e f g h i j k l m n o p',                                            # 16 tokens, all unknown but 'a' perhaps
]
text = []
for s in SENTENCES:
    idx, n = text_processing.preprocess_sentence(s, vocab, 15)
    text.append({'sentence': s, 'indices': [int(i) for i in idx], 'seq_len': int(n)})
with open(os.path.join(OUT, 'text.json'), 'w') as f:
    json.dump(text, f, indent=1)

np.savez_compressed(os.path.join(OUT, 'spatial.npz'), **{'%dx%d' % (h, w): generate_spatial_batch(1, h, w)[0] for h, w in ((8, 8), (12, 12))})


def scene(size, seed):
    """Boxes with both ends included, small masks [y2-y1+1, x2-x1+1], and a ``predicts`` chosen per instance."""
    rng = np.random.RandomState(seed)
    predicts = (rng.rand(size, size) < 0.5).astype(np.float32)
    boxes, masks = [], []

    def add(y1, x1, y2, x2, fill):
        m = fill(y2 - y1 + 1, x2 - x1 + 1)
        boxes.append([y1, x1, y2, x2])
        masks.append(np.ascontiguousarray(m, dtype=np.uint8))
        return m
    q = size // 4
    add(1, 3, q, q + 5, lambda h, w: (rng.rand(h, w) < 0.6).astype(np.uint8))                  # random over random predicts
    # exactly one half: a mask of 2 n ones, predicts set on the first n of them
    m = add(q + 2, 2, q + 5, 9, lambda h, w: np.ones((h, w), np.uint8))
    predicts[q + 2:q + 6, 2:10] = 0
    predicts[q + 2:q + 4, 2:10] = 1
    add(2, 2 * q, 9, 2 * q + 6, lambda h, w: np.zeros((h, w), np.uint8))                        # an empty mask: 0 / 0
    # bytes that are not 0 / 1: the numerator counts pixels, the denominator adds bytes
    m = add(2 * q, 2 * q + 1, 2 * q + 7, 2 * q + 8, lambda h, w: np.full((h, w), 3, np.uint8))
    predicts[2 * q:2 * q + 8, 2 * q + 1:2 * q + 9] = 1                                        # every pixel set, and still 1 / 3
    m = add(3 * q, 1, size - 1, q, lambda h, w: (rng.rand(h, w) < 0.3).astype(np.uint8) * 2)      # ends in the last row
    predicts[3 * q:size, 1:q + 1] = 1                                                           # 1 / 2 exactly: not matched
    add(3 * q + 1, 3 * q, size - 1, size - 1, lambda h, w: np.ones((h, w), np.uint8))           # the last row and column
    predicts[3 * q + 1:size, 3 * q:size] = (rng.rand(size - 3 * q - 1, size - 3 * q) < 0.9)
    add(0, 0, size - 1, size - 1, lambda h, w: (rng.rand(h, w) < 0.1).astype(np.uint8))         # the whole image
    m = add(q, 3 * q, q + 3, 3 * q + 4, lambda h, w: np.ones((h, w), np.uint8))                 # one pixel above one half
    predicts[q:q + 4, 3 * q:3 * q + 5] = 0
    predicts[q:q + 2, 3 * q:3 * q + 5] = 1
    predicts[q + 2, 3 * q] = 1
    # a grey value in predicts: the reference's stroke map keeps grey bytes, and only asks whether the product is zero
    predicts[0, 0] = 128.0
    return predicts, np.array(boxes, np.int32), masks


out = {}
for size, seed in ((64, 5), (96, 6)):
    predicts, boxes, masks = scene(size, seed)
    sdp.IMAGE_SIZE = size
    tmp = tempfile.mkdtemp()
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
                matched = sdp.get_pred_instance_mask(path, predicts.copy())[4]
                full = sdp.expand_small_segmentation_mask(masks, boxes)
                scores = [sdp.compute_mask_occupied_percentage(predicts.copy(), full[k]) for k in range(len(masks))]
        finally:
            np.load = _load
    finally:
        shutil.rmtree(tmp)
    tag = 's%d/' % size
    out[tag + 'predicts'] = predicts
    out[tag + 'boxes'] = boxes
    out[tag + 'matched'] = np.array(matched, np.int64)
    out[tag + 'scores'] = np.array(scores, np.float64)
    out[tag + 'n'] = np.array(len(masks))
    for k, m in enumerate(masks):
        out[tag + 'mask_%d' % k] = m
    print(size, 'matched', matched, 'scores', scores)
np.savez_compressed(os.path.join(OUT, 'selection.npz'), **out)
print(sum(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT)), 'bytes')
