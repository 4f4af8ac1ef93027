"""Scoring the held-out split while the matcher trains (match_main.py --mode train --val_freq F).

    once         MatchSceneCache of the val scenes (no features); every caption's tokens and its 256-byte lut on the device
    per pass     per scene  MatchModel.features(cached sketch)
                 per caption, as written in the file (no augmentation: --mode eval's default)
                            MatchModel.head -> ssc_match_score -> its row of one int64 [captions,5] device buffer
                 one wait for the device at the end; the record is arithmetic on the rows (match_eval.Totals)

The pass reads the weights of the moment and writes only buffers that a training step fills before it reads them (the model's
forward buffers, the reduction workspace, its own rows): it touches neither the generator of the tuples' order, nor the Adam
slots, nor the loss slots, and the training trajectory with it is that without it, bit for bit.

Not here: mask AP (--mode eval), a feature cache of the held-out scenes, a caption-batched head."""
import json
import os
import time

import numpy as np

from . import match_cache, match_eval, match_train, matching

LOG_NAME = 'match_validation.jsonl'


def validation_scenes(captions_base_dir, data_base_dir, val_scenes=0, split='val'):
    """The scenes a pass scores: the first ``val_scenes`` of sentence_instance_<split>.json (0: all).  A missing caption file,
    a missing ground-truth file and a caption without a word are ValueErrors; nothing but the caption file is read."""
    scenes = match_eval.read_captions(captions_base_dir, split)
    if val_scenes:
        scenes = scenes[:int(val_scenes)]
    if not scenes:
        raise ValueError('--captions_base_dir %r: no scene in the caption file of %r' % (captions_base_dir, split))
    for image_id, pairs in scenes:
        for path in match_eval.ground_truth_paths(data_base_dir, split, image_id):
            if not os.path.isfile(path):
                raise ValueError('scene %s: %s: no such file' % (image_id, path))
        for caption, _idx in pairs:
            if not matching.sentence_tokens(caption):
                raise ValueError('scene %s: the caption %r holds no word' % (image_id, caption))
    return scenes


def validation_record(iteration, scenes, rows, seconds):
    """rows: one (I, P, A, live, loss) per caption -- ssc_match_score's four counts and its summed class loss.  -> the line of
    match_validation.jsonl.  U = P + A - I (match_eval.mask_iu); the overall IoU is sum I / sum U and precision@t the share of
    the captions with I / U >= t in float64: match_eval.Totals' arithmetic."""
    totals = match_eval.Totals(mask_ap=False)
    loss, live = 0.0, 0
    for I, P, A, n_live, l in rows:
        totals.add(int(I), int(P) + int(A) - int(I))
        loss += float(l)
        live += int(n_live)
    if totals.captions < 1:
        raise ValueError('no caption was scored')
    return {'iter': int(iteration), 'scenes': int(scenes), 'captions': totals.captions, 'overall_iou': totals.overall_iou(),
            'precision': {str(t): p for t, p in zip(match_eval.IOU_LEVELS, totals.precision())},
            'class_loss_mean': loss / totals.captions, 'live_pixels': live, 'seconds': float(seconds)}


def validation_line(record):
    return 'val: iter = %d, overall IoU = %f, precision@0.5 = %f, loss = %f' % (record['iter'], record['overall_iou'],
                                                                                record['precision']['0.5'], record['class_loss_mean'])


class MatchValidation(object):
    """``scenes``: ``validation_scenes``' list.  Builds the cache of the held-out scenes (``beside``: the bytes of the caches that
    are on the device already), sends every caption through match_eval.caption_labels and uploads its tokens and its lut."""

    def __init__(self, model, vocab, scenes, data_base_dir, split='val', beside=0,
                 remedy='score fewer scenes (--val_scenes N) or none (--val_freq 0)', preview=0):
        import torch
        cfg = model.cfg
        self.model, self.scenes = model, scenes
        self.cache = match_cache.MatchSceneCache(scenes, data_base_dir, split, cfg.size, model.device, beside=beside,
                                                 remedy_scenes=remedy)
        self.plan, toks, luts = [], [], []           # per scene of the file: (its entry, [(row, seq_len), ..])
        self.texts = []                              # per caption: (scene, caption)
        for image_id, pairs in scenes:
            i = self.cache.index[image_id]
            rows = []
            for caption, inst_indices in pairs:
                labels = match_eval.caption_labels(image_id, inst_indices, int(self.cache.n_inst[i]), self.cache.area[i])
                indices, seq_len = matching.preprocess_sentence(caption, vocab, cfg.max_len)
                rows.append((len(toks), int(seq_len)))
                self.texts.append((str(image_id), caption))
                toks.append(np.asarray(indices, dtype=np.int32).reshape(-1))
                luts.append(match_train.caption_lut(labels))
            self.plan.append((i, rows))
        self.captions = len(toks)
        self.tok = torch.from_numpy(np.stack(toks)).to(model.device)
        self.lut = torch.from_numpy(np.stack(luts)).to(model.device)
        self.rows = torch.zeros((self.captions, 5), dtype=torch.int64, device=model.device)
        self.nbytes = self.cache.nbytes
        # --val_preview K: a sheet of the first K captions (preview.py); it reads the pass's buffers and writes only its own
        self.preview = None
        if preview:
            from . import preview as P
            self.preview = P.MatchPreview(model, self.captions, preview)

    def run(self, iteration):
        """One pass with the weights of the moment.  -> the record of ``validation_record``."""
        import torch
        from . import hip
        t0 = time.time()
        cache, model, pv = self.cache, self.model, self.preview
        ws = hip.workspace()
        for i, rows in self.plan:
            feat, stroke = model.features(cache.sketch[i])
            for k, seq_len in rows:
                pred = model.head(feat, self.tok[k], seq_len)
                hip.match_score(pred, cache.sketch[i], cache.labels[i], self.lut[k], out=self.rows[k], ws=ws)
                if pv is not None:
                    pv.caption(k, pred, stroke, cache.sketch[i], cache.labels[i], self.lut[k])
        host = self.rows.cpu().numpy()                  # the pass's one wait for the device
        self.last_rows = host
        loss = host[:, 0].copy().view(np.float64)
        return validation_record(iteration, len(self.plan), [(host[k, 1], host[k, 2], host[k, 3], host[k, 4], loss[k])
                                                             for k in range(self.captions)], time.time() - t0)

    def run_and_log(self, iteration, log_root, log=print):
        record = self.run(iteration)
        with open(os.path.join(log_root, LOG_NAME), 'a') as f:
            f.write(json.dumps(record) + '\n')
        if self.preview is not None:        # the sheet comes to the host here, behind the rows
            host = self.last_rows
            self.preview.write(log_root, iteration, [{'scene': s, 'caption': c, 'I': int(host[k, 1]), 'P': int(host[k, 2]),
                                                      'A': int(host[k, 3])} for k, (s, c) in enumerate(self.texts[:self.preview.n])])
        if log is not None:
            log(validation_line(record))
        return record
