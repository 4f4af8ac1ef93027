"""Scoring a held-out set during Foreground training (obj_colorization_main.py --val_freq F): every F iterations the generator,
with the weights of that moment, colours the records of data/tfrecord/val and its outputs are scored against the targets --
MAE, PSNR and SSIM, the definitions of --mode val --metrics 1 -- without leaving the device.  It stands where the reference
meant to score checkpoints (--count_inception_score_freq; its Inception call is commented out, graph_single.py:557-559).

The pass, which is the definition of the numbers it writes:
  * the records of a ``record_cache.RecordCache`` over data/tfrecord/val in cache order ((sorted file, position)), the first
    --val_records of them when that is set;
  * in batches of --batch_size, the last one short when the count is no multiple (``batch_plan``).  The generator's norms are
    batch statistics, so an image's output depends on the batch it sits in: the batching is part of the definition;
  * a batch is decoded by hip.decode_paired_cached_u8 without dequantisation noise, run through the tower's replayed inference
    graph (``generate(..., clone=False)``) with the cache's captions and class ids, and its NHWC output buffer is scored
    against the planar decoded target by hip.image_metrics_f32 -- the uint8 images are never written;
  * the generator's noise vectors come from a torch.Generator of the evaluator's own, seeded with ``NOISE_SEED`` at the start
    of every pass: every pass sees the same noise, no generator that training draws from is touched;
  * the [S,5] float64 rows come to the host once, behind the last batch.
--val_preview K: the batches that hold one of the first K records also put their outputs -- hip.image_postprocess_u8 of the pass's
own ``tower.infer_nhwc`` rows, the conversion that makes --mode val's PNGs -- into a preview sheet beside the records' sketches
and targets (preview.ForegroundPreview).  No second forward pass, no draw from a generator, and nothing
written but the preview's own buffers.
--color_metrics 1: one more launch per batch, hip.color_metrics_f32 on the same two buffers, fills [S,13] rows of colour sums
(DESIGN.md section 8.17); they come to the host behind the five-sum rows and become the line's "color" key.
"""
import time

import numpy as np
import torch

from . import metrics

NOISE_SEED = 20241  # of the generator's noise vectors, at the start of every pass
NOISE_DIM = 256


def batch_plan(records, batch_size):
    """[(first, end)] record numbers of the batches of a pass over ``records`` records: full batches in order, then the rest."""
    records, batch_size = int(records), int(batch_size)
    assert records >= 0 and batch_size >= 1
    return [(a, min(a + batch_size, records)) for a in range(0, records, batch_size)]


def record_names(cache):
    """'<category>_<image name without .png>' of every record, as --mode val names its files, and the categories."""
    stems = [n[:-4] if n.endswith('.png') else n for n in cache.name]
    return ['%s_%s' % (c, n) for c, n in zip(cache.category, stems)], list(cache.category)


def pass_noise(gen, n, device):
    """The noise vectors of the next batch of n images from the pass's generator."""
    return torch.randn((n, NOISE_DIM), device=device, generator=gen)


def validation_line(step, names, groups, rows, seconds, color_rows=None):
    """(the log/validation.jsonl entry of one pass, the metrics.summarise summary it was cut from).  color_rows ([S,13], the
    pass's colour sums under --color_metrics 1) adds the key 'color': the all and per-category levels of
    metrics.summarise_color."""
    summary = metrics.summarise(names, groups, rows)
    line = {'step': int(step), 'images': len(names), 'all': summary['all'], 'groups': summary['groups'],
            'seconds': float(seconds)}
    if color_rows is not None:
        c = metrics.summarise_color(names, groups, color_rows)
        line['color'] = {'all': c['all'], 'groups': c['groups']}
    return line, summary


class HeldOutEvaluator(object):
    """``run(tower)`` is one pass; the record numbers and class ids are uploaded once, here."""

    def __init__(self, cache, batch_size, preview=0, color=False):
        self.cache, self.batch_size = cache, int(batch_size)
        self.color_rows = self.color_host = None        # --color_metrics 1: the [S,13] colour sums, on the device and of the last pass
        self.preview = None
        if preview:
            from .preview import ForegroundPreview
            self.preview = ForegroundPreview(cache, preview)
        self.plan = batch_plan(len(cache), batch_size)
        self.names, self.groups = record_names(cache)
        dev = cache.device
        self.numbers = torch.arange(len(cache), dtype=torch.int32, device=dev)
        self.class_id = torch.from_numpy(np.ascontiguousarray(cache.class_id, dtype=np.int32)).to(dev)
        self.rows = torch.empty((len(cache), 5), dtype=torch.float64, device=dev)
        self.gen = torch.Generator(device=dev)
        if color:
            self.color_rows = torch.empty((len(cache), 13), dtype=torch.float64, device=dev)

    def run(self, tower):
        """-> ([S,5] float64 rows on the host, seconds).  Everything is launched on the current stream, behind whatever
        training has queued there; the caller has settled every pending step."""
        from . import hip
        t0 = time.time()
        cache, pv = self.cache, self.preview
        self.gen.manual_seed(NOISE_SEED)
        if pv is not None:
            pv.start()
        for a, b in self.plan:
            target, sketch = hip.decode_paired_cached_u8(cache, self.numbers[a:b], cache.size, noise=None)
            noise_vec = pass_noise(self.gen, b - a, cache.device)
            tower.generate(sketch, cache.text[a:b], noise_vec, labels=self.class_id[a:b], clone=False)
            out, coff = tower.infer_nhwc
            hip.image_metrics_f32(out, coff, target, out=self.rows[a:b])
            if self.color_rows is not None:
                hip.color_metrics_f32(out, coff, target, out=self.color_rows[a:b])
            if pv is not None:
                pv.batch(out, coff, a, b)
        rows = self.rows.cpu().numpy()      # the one copy to the host (it waits for the pass)
        if self.color_rows is not None:
            self.color_host = self.color_rows.cpu().numpy()
        hip.check_sk('held-out pass')
        return rows, time.time() - t0
