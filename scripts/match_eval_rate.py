#!/usr/bin/env python
"""What scoring one scene costs at the released size (match_main.py --mode eval).

One process, a MatchModel of the released configuration (768 x 768, units 3 / 4 / 23 / 3, 1000 / 1000 / 500) with random weights
(the cost does not depend on them), a synthetic sketch, a label map of --gt instances and --instances predicted boxes with random
masks, --captions captions of --words words.  After --warmup scenes, per scene and between device events on the stream:

  features       the input copy, ssc_match_preprocess_u8, the backbone, the copy of the feature map: once per scene
  predict        head + ssc_match_finish: per caption
  label_hist     ssc_label_hist_u8 at size x size, without and with a gate: each alone
  instance_hist  ssc_instance_label_hist over the predicted instances: alone
  score          per caption: ssc_instance_occupancy + ssc_label_hist_u8(labels, predicts), the two read-backs and the host
                 arithmetic (wall clock)
  forward        the same captions through MatchModel.forward, one whole pass per caption: the reference's schedule

Medians over --reps scenes.  Writes --out (default profiles/match_eval.txt).  A record of one run on one box, not a threshold."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    return a, b, out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--size', type=int, default=768)
    ap.add_argument('--gt', type=int, default=12)
    ap.add_argument('--instances', type=int, default=16)
    ap.add_argument('--captions', type=int, default=5)
    ap.add_argument('--words', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'match_eval.txt'))
    args = ap.parse_args()
    from sketchyscenecolorization_amd import hip, match_eval, matching
    if not torch.cuda.is_available():
        raise SystemExit('match_eval_rate.py measures on the device: no GPU here')
    cfg = matching.MatchConfig(size=args.size)
    model = matching.MatchModel(cfg)
    model.init_random(1)
    rng = np.random.RandomState(0)
    s = cfg.size
    sketch = np.full((s, s, 3), 255, np.uint8)
    sketch[rng.rand(s, s) < 0.1] = 0
    labels = np.zeros((s, s), np.uint8)
    for k in range(args.gt):
        y, x = rng.randint(0, s - s // 4, 2)
        labels[y:y + rng.randint(s // 10, s // 4), x:x + rng.randint(s // 10, s // 4)] = k + 1
    n_inst = int(labels.max())
    boxes, masks = [], []
    for _ in range(args.instances):
        y1, x1 = rng.randint(0, s - s // 3, 2)
        y2, x2 = y1 + rng.randint(s // 8, s // 3), x1 + rng.randint(s // 8, s // 3)
        boxes.append([y1, x1, y2, x2])
        masks.append((rng.rand(y2 - y1 + 1, x2 - x1 + 1) < 0.3).astype(np.uint8))
    boxes = np.array(boxes, np.int32)
    buf, offsets = matching.pack_masks(boxes, masks, s)
    vocab = {w: k for k, w in enumerate(['<pad>', '<unk>'] + ['w%d' % k for k in range(cfg.vocab_size - 2)])}
    sentences = [matching.preprocess_sentence(' '.join('w%d' % ((c + k) % (cfg.vocab_size - 2)) for k in range(args.words)), vocab,
                                              cfg.max_len) for c in range(args.captions)]
    present = [int(g) - 1 for g in np.unique(labels) if g]
    targets = [[present[(c + k) % len(present)] for k in range(2)] for c in range(args.captions)]
    t = {k: [] for k in ('features', 'predict', 'hist', 'hist_gated', 'instance_hist', 'score', 'forward')}
    for rep in range(args.warmup + args.reps):
        scene = match_eval.SceneOnDevice('rate', labels, boxes, buf, offsets, n_inst)
        ev = {'hist': _timed(lambda: hip.label_hist_u8(scene.labels)),
              'instance_hist': _timed(lambda: hip.instance_label_hist(scene.labels, scene.buf, scene.boxes, scene.offsets)),
              'features': _timed(lambda: model.features(sketch))}
        feat, stroke = ev['features'][2]
        per_caption, score = [], []
        for (indices, seq_len), target in zip(sentences, targets):
            a, b, (_up, predicts) = _timed(lambda: model.predict(feat, stroke, indices, seq_len))
            per_caption.append((a, b))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            match_eval.score_caption(predicts, scene, target)
            score.append((time.perf_counter() - t0) * 1e3)
        ev['hist_gated'] = _timed(lambda: hip.label_hist_u8(scene.labels, predicts))
        forward = [_timed(lambda: model.forward(sketch, indices, seq_len))[:2] for indices, seq_len in sentences]
        torch.cuda.synchronize()
        if rep >= args.warmup:
            for k in ('features', 'hist', 'hist_gated', 'instance_hist'):
                t[k].append(ev[k][0].elapsed_time(ev[k][1]))
            t['predict'] += [a.elapsed_time(b) for a, b in per_caption]
            t['forward'] += [a.elapsed_time(b) for a, b in forward]
            t['score'] += score
    med = {k: statistics.median(v) for k, v in t.items()}
    c = args.captions

    def row(text, k):
        return '%-74s %9.3f ms  (min %.3f, max %.3f)' % (text, med[k], min(t[k]), max(t[k]))
    lines = ['match_eval_rate.py: one scene at %d x %d, %d captions of %d words, %d ground-truth and %d predicted instances, random '
             'weights; medians of %d scenes after %d warm-up, device events; %s, library %s'
             % (s, s, c, args.words, n_inst, len(masks), args.reps, args.warmup, torch.cuda.get_device_name(0), hip.build_hash()),
             row('features, once per scene (input copy, preprocess, backbone, feature copy)', 'features'),
             row('predict, per caption (head + ssc_match_finish)', 'predict'),
             row('ssc_label_hist_u8 at %d x %d, no gate' % (s, s), 'hist'),
             row('ssc_label_hist_u8 at %d x %d, gated by predicts' % (s, s), 'hist_gated'),
             row('ssc_instance_label_hist, %d instances' % len(masks), 'instance_hist'),
             row('score_caption, per caption (two kernels, two read-backs, host arithmetic; wall clock)', 'score'),
             row('MatchModel.forward, per caption (the whole network: the reference\'s schedule)', 'forward'),
             'a scene of %d captions: features + %d x predict = %.3f ms; %d x forward = %.3f ms'
             % (c, c, med['features'] + c * med['predict'], c, c * med['forward']),
             'Measured once on one box: a record, no comparison with anything earlier.']
    print('\n'.join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    model.close()


if __name__ == '__main__':
    main()
