"""Scoring a held-out set during Background training (bg_colorization_main.py --val_freq F): every F steps the generator, with the
weights of that moment, colours the scenes of ``<data_base_dir>/{foreground,background,segment}/val`` (captions/val.json) and
two things are scored without leaving the device: its image against the scene's background -- MAE, PSNR and SSIM, the
definitions of --mode test --metrics 1 -- and its region logits against the scene's labels -- pixel accuracy and IoU.

The pass, which is the definition of the numbers it writes:
  * the records of captions/val.json in file order, the first --val_records of them when that is set, held in a
    ``scene_cache.SceneCache`` of their own on the trainer's device;
  * ONE scene per forward pass, as test mode: the generator's norms are batch statistics, so a score does not depend on
    --batch_size;
  * per scene hip.bg_stage_cached_u8 on one slot row (nothing recoloured) makes the float input and the int32 labels, then
    ``G.forward(x, tokens, None, TAG)`` runs under a buffer tag no training step uses: a forward pass at another batch shape
    under a training tag would reallocate buffers that the captured training graphs point into;
  * hip.image_metrics_bg_f32 scores the float image against the cache's background entry; the cache's foreground and segment
    entries are the paste-back source and the mask (the pasted-back foreground pixels are not counted), and the quantisation
    is test mode's floor(clamp((x+1)/2, 0, 1)*255 + 0.5): the rows are the bits of image_metrics_u8(bg_finish_u8(...)) of the
    PNG that --mode test would write for the scene;
  * hip.seg_confusion counts (label, prediction) pairs of the region logits against the staged labels;
  * the [S,5] float64 rows and the [S,K*K+1] int64 rows come to the host once, behind the last scene.
It draws nothing from ``random`` or a torch generator and writes no parameter, optimizer slot or scalars.jsonl entry.
--val_preview K: the first K scenes also go into a preview sheet -- the foreground, hip.bg_finish_u8 of the pass's own float image
(the bytes --mode test would write) and the background (preview.BackgroundPreview) -- written as
log/previews/step_<n>.png and .json; it reads the pass's buffers and writes only its own.
--color_metrics 1: one more launch per scene, hip.color_metrics_bg_f32 on the arguments of hip.image_metrics_bg_f32, fills [S,13]
rows of colour sums; they become the line's "color" key.
"""
import json
import os
import time

import numpy as np
import torch

from . import metrics

TAG = 'bgval'       # the buffer tag of the pass's forward passes (training uses 'bg', 'dr', 'df', 'dg')


def held_out_scenes(p, scenes_class):
    """The ``Scenes`` of mode 'val' under p['data_base_dir'] and the record numbers of a pass (the first --val_records, or
    all), or (None, None) -- with one printed line -- when captions/val.json is missing.  A record without a segment file is
    refused here, by name: the region score and the mask both need it."""
    cap = os.path.join(p['data_base_dir'], 'captions', 'val.json')
    if not os.path.exists(cap):
        print('%s not found: training without held-out passes (--val_freq %d ignored)' % (cap, p['val_freq']))
        return None, None
    scenes = scenes_class(dict(p, mode='val'))
    n = len(scenes) if not p.get('val_records', 0) else min(int(p['val_records']), len(scenes))
    if n < 1:
        raise ValueError('%s holds no record: nothing to score with --val_freq %d' % (cap, p['val_freq']))
    for i in range(n):
        seg = os.path.join(scenes.dirs['segment'], scenes.records[i]['fg_name'])
        if not os.path.exists(seg):
            raise ValueError('held-out record %d has no segment file %s: the region score and the mask of a held-out pass '
                             'need it' % (i, seg))
    return scenes, range(n)


def build_cache(scenes, keep, device, beside=0):
    """The held-out ``SceneCache``; ``beside`` = the bytes of the training cache, which count against the same limit."""
    from . import scene_cache
    cache = scene_cache.SceneCache(scenes, device, keep=keep, beside=beside,
                                   remedy='score fewer held-out records (--val_records) or run with --scene_cache off')
    print('held-out cache: %d scenes from %d foregrounds, %d backgrounds, %d segment maps; %.1f MB on %s, built in %.1f s'
          % (len(cache), cache.fg.shape[0], cache.bg.shape[0], cache.seg.shape[0], cache.nbytes / 1e6, cache.device,
             cache.build_seconds))
    return cache


def scene_names(scenes, keep):
    """The names --mode test gives the scenes' files: the background's name without its extension."""
    return [scenes.records[i]['bg_name'][:-4] for i in keep]


def validation_line(step, names, rows, conf, seconds, color_rows=None):
    """(the log/validation.jsonl entry of one pass, the metrics.summarise summary it was cut from).  color_rows ([S,13], the
    pass's colour sums under --color_metrics 1) adds the key 'color': the all and group levels of metrics.summarise_color."""
    summary = metrics.summarise(names, ['all'] * len(names), rows)
    line = {'step': int(step), 'images': len(names), 'all': summary['all'], 'groups': summary['groups'],
            'region': metrics.region_scores(conf), 'seconds': float(seconds)}
    if color_rows is not None:
        c = metrics.summarise_color(names, ['all'] * len(names), color_rows)
        line['color'] = {'all': c['all'], 'groups': c['groups']}
    return line, summary


def dumps_line(line):
    """The text of one log/validation.jsonl entry: sorted keys, so that equal passes write equal lines."""
    return json.dumps(line, sort_keys=True) + '\n'


def printed_line(line, summary):
    fmt = lambda v: 'n/a' if v is None else '%.4f' % v      # noqa: E731
    return 'held-out pass at step %d: %s  region miou %s accuracy %s' % (
        line['step'], metrics.all_line(summary), fmt(line['region']['miou']), fmt(line['region']['accuracy']))


class HeldOutEvaluator(object):
    """``run(trainer)`` is one pass over ``cache``; the slot rows are uploaded once, here."""

    def __init__(self, cache, names, seg_classes, preview=0, color=False):
        assert len(names) == len(cache)
        self.color_rows = self.color_host = None        # --color_metrics 1: the [S,13] colour sums, on the device and of the last pass
        self.preview = None
        if preview:
            from .preview import BackgroundPreview
            self.preview = BackgroundPreview(cache, preview)
        self.cache, self.names, self.K = cache, list(names), int(seg_classes)
        dev, S = cache.device, len(cache)
        H, W = cache.fg.shape[1:3]
        self.slots = torch.from_numpy(np.ascontiguousarray(cache.slots, dtype=np.int32)).to(dev)
        self.x = torch.empty((1, H, W, 3), dtype=torch.float32, device=dev)
        self.y = torch.empty_like(self.x)       # the stage kernel's other outputs: written, not read
        self.xd = torch.empty((1, H, W, 8), dtype=torch.float32, device=dev)
        self.count = torch.empty(1, dtype=torch.float32, device=dev)
        self.labels = torch.empty((1, H, W), dtype=torch.int32, device=dev)
        self.rows = torch.empty((S, 5), dtype=torch.float64, device=dev)
        self.conf = torch.empty((S, self.K * self.K + 1), dtype=torch.int64, device=dev)
        if color:
            self.color_rows = torch.empty((S, 13), dtype=torch.float64, device=dev)

    def run(self, tr):
        """-> ([S,5] float64 rows, [S,K*K+1] int64 counts, seconds), on the host.  Everything is launched on the current stream,
        behind whatever training has queued there; the caller has settled every pending step."""
        from . import hip
        t0 = time.time()
        c = self.cache
        for i in range(len(c)):
            hip.bg_stage_cached_u8(c.fg, c.bg, c.seg, self.slots[i:i + 1], None, self.x, self.y, self.xd, self.labels, self.count)
            gctx = tr.G.forward(self.x, c.tokens[i:i + 1], None, TAG)
            sf, sb, ss = (int(v) for v in c.slots[i])
            hip.image_metrics_bg_f32(gctx['image'], c.fg[sf:sf + 1], c.bg[sb:sb + 1], c.seg[ss:ss + 1], out=self.rows[i:i + 1])
            hip.seg_confusion(gctx['region_logits'], self.labels, self.K, out=self.conf[i:i + 1])
            if self.color_rows is not None:
                hip.color_metrics_bg_f32(gctx['image'], c.fg[sf:sf + 1], c.bg[sb:sb + 1], c.seg[ss:ss + 1],
                                         out=self.color_rows[i:i + 1])
            if self.preview is not None:
                self.preview.scene(i, gctx['image'])
        rows = self.rows.cpu().numpy()      # the two copies to the host (the first waits for the pass)
        conf = self.conf.cpu().numpy()
        if self.color_rows is not None:
            self.color_host = self.color_rows.cpu().numpy()
        return rows, conf, time.time() - t0


def open_held_out(p, scenes_class, tr, beside=0):
    """What ``--val_freq`` sets up at the start of training: the evaluator over the held-out cache, or None without the set."""
    scenes, keep = held_out_scenes(p, scenes_class)
    if scenes is None:
        return None
    cache = build_cache(scenes, keep, tr.losses.device, beside)
    return HeldOutEvaluator(cache, scene_names(scenes, keep), p['seg_classes'], preview=p.get('val_preview', 0),
                            color=bool(p.get('color_metrics', 0)))


def run_pass(ev, tr, log_dir):
    """One pass behind a finished step: a line appended to log/validation.jsonl and one printed."""
    tr.loss_values()        # the step has finished (its losses are on the host) before the pass is queued behind it
    rows, conf, seconds = ev.run(tr)
    line, summary = validation_line(tr.global_step, ev.names, rows, conf, seconds, getattr(ev, 'color_host', None))
    with open(os.path.join(log_dir, 'validation.jsonl'), 'a') as fp:
        fp.write(dumps_line(line))
    if ev.preview is not None:      # the sheet comes to the host behind the rows
        ev.preview.write(log_dir, tr.global_step, ev.names)
    print(printed_line(line, summary))
    if 'color' in line:     # --color_metrics 1
        print('held-out pass at step %d: %s' % (line['step'], metrics.color_line(line['color'])))
    return line
