#!/usr/bin/env python
"""What one training iteration of the matcher's fusion head costs at the released size (match_main.py --mode train, DESIGN.md
section 8.8).

One process, a MatchModel of the released configuration (768 x 768, units 3 / 4 / 23 / 3, 1000 / 1000 / 500) with a random backbone
and a fresh head (the cost does not depend on the weights), a synthetic sketch and label map, a sentence of --words words.  After
--warmup iterations, per iteration and between device events on the stream:

  backbone   MatchModel.features: the input copy, ssc_match_preprocess_u8, the frozen backbone, the copy of the feature map
  head       MatchTrainer.head_train: the head's forward pass with every step's state kept
  loss       ssc_match_loss_grad (two launches) on the 768 x 768 sketch and label map
  backward   MatchTrainer.backward: ssc_squash_project_bwd, BPTT of both cells, every filter gradient
  optimiser  ssc_l2_reg on the two DW, ssc_adam_tf per tensor, the refresh of the bf16 planes

and the whole iteration through MatchTrainer.step (uploads included) between device events.  Medians over --reps iterations.
Writes --out (default profiles/match_train.txt).  A record of one run on one box, not a threshold."""
import argparse
import os
import statistics
import sys

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
    ap.add_argument('--words', type=int, default=9)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'match_train.txt'))
    args = ap.parse_args()
    from sketchyscenecolorization_amd import hip, match_train, matching
    if not torch.cuda.is_available():
        raise SystemExit('match_train_rate.py measures on the device: no GPU here')
    cfg = matching.MatchConfig(size=args.size)
    if not 1 <= args.words <= cfg.max_len:
        raise SystemExit('--words %d: 1 .. %d' % (args.words, cfg.max_len))
    model = matching.MatchModel(cfg)
    variables = matching.random_variables(cfg, 1)
    variables.update(match_train.init_head(cfg, 1))
    model.load_dict(variables)
    trainer = match_train.MatchTrainer(model)
    rng = np.random.RandomState(0)
    s = cfg.size
    sketch = np.full((s, s, 3), 255, np.uint8)
    sketch[rng.rand(s, s) < 0.1] = 0
    labels = np.zeros((s, s), np.uint8)
    for k in range(12):
        y, x = rng.randint(0, s - s // 4, 2)
        labels[y:y + rng.randint(s // 10, s // 4), x:x + rng.randint(s // 10, s // 4)] = k + 1
    lut = match_train.caption_lut([int(g) for g in np.unique(labels)[1:3]])
    idx = np.zeros(cfg.max_len, np.int64)
    idx[:args.words] = 2 + np.arange(args.words) % (cfg.vocab_size - 2)
    scene = {'sketch': sketch, 'labels': labels}
    parts = ('backbone', 'head', 'loss', 'backward', 'optimiser')
    t = {k: [] for k in parts + ('step',)}
    tok = torch.from_numpy(idx.astype(np.int32)).cuda()
    lut_d = torch.from_numpy(lut).cuda()
    for rep in range(args.warmup + args.reps):
        ev = {}
        ev['backbone'] = _timed(lambda: model.features(sketch))
        feat = ev['backbone'][2][0]
        sketch_d = model._buf('sketch', (s, s, 3), torch.uint8)
        labels_d = trainer.upload_scene(labels)
        ev['head'] = _timed(lambda: trainer.head_train(feat, tok, args.words))
        pred = ev['head'][2]
        ev['loss'] = _timed(lambda: trainer.loss_and_grad(pred, sketch_d, labels_d, lut_d))
        dpred = ev['loss'][2]
        ev['backward'] = _timed(lambda: trainer.backward(dpred))
        ev['optimiser'] = _timed(lambda: trainer.apply(2.5e-4))
        ev['step'] = _timed(lambda: trainer.step(scene, lut, idx, args.words, 2.5e-4))
        torch.cuda.synchronize()
        if rep >= args.warmup:
            for k in t:
                t[k].append(ev[k][0].elapsed_time(ev[k][1]))
    loss = trainer.last_loss()
    med = {k: statistics.median(v) for k, v in t.items()}
    gates = cfg.max_len * cfg.feat * cfg.feat * 4 * model.cm * 4
    states = 2 * (cfg.max_len + 1) * cfg.feat * cfg.feat * model.cm * 4

    def row(text, k):
        return '%-86s %9.3f ms  (min %.3f, max %.3f)' % (text, med[k], min(t[k]), max(t[k]))
    lines = ['match_train_rate.py: one iteration at %d x %d, a sentence of %d words, random backbone, fresh head; medians of %d '
             'iterations after %d warm-up, device events; %s, library %s'
             % (s, s, args.words, args.reps, args.warmup, torch.cuda.get_device_name(0), hip.build_hash()),
             row('backbone (input copy, preprocess, frozen backbone, feature copy)', 'backbone'),
             row('head forward, every state kept (head_train)', 'head'),
             row('loss and its gradient on the 1/8 map (ssc_match_loss_grad)', 'loss'),
             row('backward (ssc_squash_project_bwd, BPTT of both cells, filter gradients)', 'backward'),
             row('optimiser (ssc_l2_reg x 2, ssc_adam_tf x 14, refresh of the bf16 planes)', 'optimiser'),
             'the five parts together: %.3f ms' % sum(med[k] for k in parts),
             row('MatchTrainer.step, the whole iteration with its uploads', 'step'),
             'kept for the backward pass at this size (allocated once, for %d steps): %.2f GB of activated gates, %.2f GB of cell '
             'states and outputs; %.2f GB of gate gradients' % (cfg.max_len, gates / 1e9, states / 1e9, gates / 1e9),
             'the class loss of the last iteration: %.6g (finite: %s)' % (loss, bool(np.isfinite(loss))),
             'Measured once on one box: a record, no comparison with anything earlier.']
    print('\n'.join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    model.close()


if __name__ == '__main__':
    main()
