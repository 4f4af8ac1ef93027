"""Device-resident scene cache of Background training (bg_colorization_main.py --scene_cache device).

The training set repeats its files: data_preparation/bg_data_generation.py writes ``aug_num`` further records per base scene
that share its foreground and segment map.  ``SceneCache`` decodes every distinct file once, keeps the bytes on the device as
uint8 and maps each record to its three entries, so that a train step is a gather by index (hip.bg_stage_cached_u8 inside
BGTrainer.train_step_cached) and no image crosses the host-device link after start-up.
"""
import os
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

MAX_WORKERS = 16


def _seg_red(path, size):
    """The red channel of a segment png, as load_region_mask reads it (image_processing.py:14-25): not resized, so any other
    size than the images' is refused."""
    from PIL import Image
    seg = np.array(Image.open(path).convert('RGB'), dtype=np.uint8)[:, :, 0]
    if seg.shape != (size, size):
        raise ValueError('%s is %d x %d, the images are loaded at %d x %d: segment maps are not resized (load_region_mask does '
                         'not resize them either), so the scene cache takes them at --image_size only'
                         % (path, seg.shape[1], seg.shape[0], size, size))
    return np.ascontiguousarray(seg)


class SceneCache(object):
    """fg, bg uint8 [S,H,W,3] and seg uint8 [S,H,W] (the segment png's red channel: 0 / 128 / 255) on ``device``; ``slots``
    int32 [len, 3] = the fg, bg and seg entry of each cached record and ``tokens`` int32 [len, T] its caption.

    ``scenes``: the command line's ``Scenes`` (records, dirs, vocab, size, T, get).  ``keep``: the indices of the records to
    cache, in the order they are numbered here (default: all).  Without records (the synthetic scenes) every scene is cached
    as one entry of each kind, its labels stored as the segment values they stand for.  ``beside``: the bytes of the caches that
    live on the device already and count against the same limit (the training cache, when this one is the held-out set's);
    ``remedy``: what the refusal tells the user to do."""

    def __init__(self, scenes, device='cuda', keep=None, beside=0, remedy='run with --scene_cache off'):
        t0 = time.time()
        self.device = torch.device(device)
        size = scenes.size
        keep = list(range(len(scenes))) if keep is None else list(keep)
        if scenes.records is None:
            names = [[str(i) for i in keep]] * 3
            got = [scenes.get(i) for i in keep]
            self.tokens = np.concatenate([g[2] for g in got], 0).astype(np.int32)
            seg_of = np.array([0, 128, 255], np.uint8)
            loaders = [lambda k: got[k][0][0], lambda k: got[k][1][0], lambda k: seg_of[got[k][3][0]]]
            keys = [list(range(len(keep)))] * 3
            self.slots = np.repeat(np.arange(len(keep), dtype=np.int32)[:, None], 3, 1)
        else:
            from .data_processing.image_processing import load_image
            from .data_processing.text_processing import preprocess_sentence
            recs = [scenes.records[i] for i in keep]
            per_kind = [[r['fg_name'] for r in recs], [r['bg_name'] for r in recs], [r['fg_name'] for r in recs]]
            names = [sorted(set(k)) for k in per_kind]
            entry = [{n: i for i, n in enumerate(k)} for k in names]
            self.slots = np.array([[entry[k][per_kind[k][r]] for k in range(3)] for r in range(len(recs))], np.int32).reshape(-1, 3)
            self.tokens = np.array([preprocess_sentence(r['color_text'], scenes.vocab, scenes.T) for r in recs], np.int32)
            d = scenes.dirs
            loaders = [lambda n: load_image(os.path.join(d['foreground'], n), size)[0],
                       lambda n: load_image(os.path.join(d['background'], n), size)[0],
                       lambda n: _seg_red(os.path.join(d['segment'], n), size)]
            keys = names
        self.names = names
        P = size * size
        self.nbytes = (len(keys[0]) + len(keys[1])) * P * 3 + len(keys[2]) * P
        if self.device.type == 'cuda':
            # the caches together may take half of what was free before the first of them was built
            free = torch.cuda.mem_get_info(self.device)[0] + int(beside)
            if self.nbytes + int(beside) > free // 2:
                raise RuntimeError('the scene cache needs %d bytes (%d foregrounds, %d backgrounds, %d segment maps at %d x %d)%s, '
                                   'more than half of the %d bytes free on the device: %s'
                                   % (self.nbytes, len(keys[0]), len(keys[1]), len(keys[2]), size, size,
                                      ' beside the %d bytes of the cache that is there already' % beside if beside else '',
                                      free, remedy))
        shapes = [(len(keys[0]), size, size, 3), (len(keys[1]), size, size, 3), (len(keys[2]), size, size)]
        self.fg, self.bg, self.seg = [torch.empty(s, dtype=torch.uint8, device=self.device) for s in shapes]
        # each distinct file is decoded once, a few at a time; the decoded array goes straight into its entry
        with ThreadPoolExecutor(max_workers=MAX_WORKERS) as pool:
            for dst, load, ks in zip((self.fg, self.bg, self.seg), loaders, keys):
                for i, arr in enumerate(pool.map(load, ks)):
                    dst[i].copy_(torch.from_numpy(np.ascontiguousarray(arr)))
        self.build_seconds = time.time() - t0

    def __len__(self):
        return len(self.slots)
