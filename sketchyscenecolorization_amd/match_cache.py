"""Device-resident scene cache of the matcher (match_main.py --mode train --scene_cache {device, features}, and the held-out set of
--val_freq).

The train split repeats its scenes: sentence_instance_train.json holds 30 120 (scene, caption) tuples over 1337 scenes, and
match_eval.load_ground_truth -- a loadmat, a png decode with a NEAREST resize, a zoom(order=0) -- gives the same bytes every
time.  ``MatchSceneCache`` reads every distinct scene once, keeps the sketch and the label map on the device as uint8 and the
instance count and the label areas (ssc_label_hist_u8, one launch per scene) on the host, so that an iteration is
``entry(i)`` -> MatchTrainer.step and no image crosses the host-device link after start-up.  With ``features`` it also keeps the
frozen backbone's output of every scene, which depends on nothing else while only the fusion head trains.
"""
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import match_eval

MAX_WORKERS = 16


def distinct_scenes(scenes):
    """match_eval.read_captions' list -> (the image ids in the order of their first appearance, {image id: its entry})."""
    ids, index = [], {}
    for image_id, _pairs in scenes:
        if image_id not in index:
            index[image_id] = len(ids)
            ids.append(image_id)
    return ids, index


def cache_bytes(n, size, feat_channels=None):
    """-> (the bytes of n scenes: sketch uint8 [S,S,3] and labels uint8 [S,S]; the bytes of their features float
    [S/8,S/8,feat_channels], 0 without).  At 768 x 768: 2 359 296 per scene, 75 497 472 per feature map of 2048 channels."""
    n, size = int(n), int(size)
    scene = n * size * size * 4
    feat = 0 if feat_channels is None else n * (size // 8) * (size // 8) * int(feat_channels) * 4
    return scene, feat


def check_budget(scene_bytes, feature_bytes, free_before, remedy_scenes='run with --scene_cache off',
                 remedy_features='run with --scene_cache device'):
    """The memory rule of scene_cache.SceneCache: everything that is cached may together take half of what was free on the
    device before the first cache was built (``free_before``).  ValueError otherwise, naming the bytes wanted, the bytes free and
    the remedy: the scenes alone not fitting is one case, the features not fitting beside them the other."""
    scene_bytes, feature_bytes, free_before = int(scene_bytes), int(feature_bytes), int(free_before)
    limit = free_before // 2
    if scene_bytes > limit:
        raise ValueError('the scene cache needs %d bytes, more than half of the %d bytes free on the device: %s'
                         % (scene_bytes, free_before, remedy_scenes))
    if scene_bytes + feature_bytes > limit:
        raise ValueError('the feature cache needs %d bytes beside the %d bytes of the scenes, together more than half of the %d bytes '
                         'free on the device: %s' % (feature_bytes, scene_bytes, free_before, remedy_features))


class MatchSceneCache(object):
    """``scenes``: match_eval.read_captions' list (cut to what is wanted); every distinct scene of it is read once through
    match_eval.load_ground_truth (its ValueErrors pass through), on at most 16 threads.

    On the device: ``sketch`` uint8 [n,S,S,3], ``labels`` uint8 [n,S,S] and, with ``features`` = a loaded MatchModel, ``feat``
    float [n,S/8,S/8,feat_channels]: entry i is model.features(sketch[i]) copied, so build the cache after the weights are loaded.
    On the host: ``n_inst`` int64 [n], ``area`` int64 [n,256] (ssc_label_hist_u8 of every label map).
    ``beside``: the bytes of the caches that are on the device already and count against the same limit;
    ``remedy_scenes`` / ``remedy_features``: what the refusal tells the user to do."""

    def __init__(self, scenes, data_base_dir, split, size, device='cuda', features=None, beside=0,
                 remedy_scenes='run with --scene_cache off', remedy_features='run with --scene_cache device'):
        import torch
        from . import hip
        t0 = time.time()
        self.device = torch.device(device)
        self.size, self.split = int(size), str(split)
        self.ids, self.index = distinct_scenes(scenes)
        n, S = len(self.ids), self.size
        if n < 1:
            raise ValueError('no scene to cache')
        if S < 8 or S % 8:
            raise ValueError('the scene cache holds scenes of a side that is a multiple of 8, not %d' % S)
        channels = None
        if features is not None:
            if not features.loaded:
                raise RuntimeError('the matcher has no weights: the feature cache is built after they are loaded')
            if features.cfg.size != S:
                raise ValueError('the model reads scenes of %d, the cache holds %d' % (features.cfg.size, S))
            channels = features.cfg.feat_channels
        self.scene_bytes, self.feature_bytes = cache_bytes(n, S, channels)
        self.nbytes = self.scene_bytes + self.feature_bytes
        if self.device.type == 'cuda':
            free = torch.cuda.mem_get_info(self.device)[0] + int(beside)
            check_budget(self.scene_bytes + int(beside), self.feature_bytes, free, remedy_scenes, remedy_features)
        self.sketch = torch.empty((n, S, S, 3), dtype=torch.uint8, device=self.device)
        self.labels = torch.empty((n, S, S), dtype=torch.uint8, device=self.device)
        area_d = torch.empty((n, 256), dtype=torch.int64, device=self.device)
        self.n_inst = np.zeros(n, dtype=np.int64)

        def load(image_id):
            return match_eval.load_ground_truth(data_base_dir, self.split, image_id, S)
        # each distinct scene is decoded once, a few at a time; the decoded arrays go straight into their entries
        with ThreadPoolExecutor(max_workers=min(MAX_WORKERS, n)) as pool:
            for i, gt in enumerate(pool.map(load, self.ids)):
                self.sketch[i].copy_(torch.from_numpy(gt['sketch']))
                self.labels[i].copy_(torch.from_numpy(gt['labels']))
                self.n_inst[i] = gt['n_inst']
                hip.label_hist_u8(self.labels[i], out=area_d[i])
        self.area = area_d.cpu().numpy()
        self.scene_seconds = time.time() - t0
        self.feat = None
        if features is not None:
            f = S // 8
            self.feat = torch.empty((n, f, f, channels), dtype=torch.float32, device=self.device)
            for i in range(n):
                feat, _stroke = features.features(self.sketch[i])
                self.feat[i].copy_(feat[0])
            torch.cuda.synchronize(self.device)
        self.build_seconds = time.time() - t0

    def __len__(self):
        return len(self.ids)

    def entry(self, i):
        """The scene argument of MatchTrainer.step in its device-resident form: views of entry i (``i``: its number, or its image
        id)."""
        i = self.index[i] if isinstance(i, str) else int(i)
        e = {'image_id': self.ids[i], 'n_inst': int(self.n_inst[i]), 'sketch_d': self.sketch[i], 'labels_d': self.labels[i]}
        if self.feat is not None:
            e['feat_d'] = self.feat[i:i + 1]
        return e
