#!/usr/bin/env python
"""What one instance match costs at the released size (match_main.py).

One process, a MatchModel of the released configuration (768 x 768, units 3 / 4 / 23 / 3, 1000 / 1000 / 500) with random weights
(the cost does not depend on them), a synthetic sketch and --instances boxes with random masks.  After --warmup passes, per
repetition and between device events on the stream:

  backbone    the input copy, ssc_match_preprocess_u8, the convs, the max-pool, the units, the four rearrangements
  head        projection, l2 norms, both LSTMs over the sentence's words, ssc_squash_project
  finish      ssc_match_finish and ssc_instance_occupancy (masks already on the device)

and by the wall clock: load (random weights made on the host, folded, padded and uploaded -- a checkpoint read replaces the
first part) and one whole match_instances call (with the mask upload and the read-back of counts, up and predicts).
Medians over --reps.  Writes --out (default profiles/match.txt).  A record of one run on one box, not a threshold."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--size', type=int, default=768)
    ap.add_argument('--instances', type=int, default=16)
    ap.add_argument('--words', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'match.txt'))
    args = ap.parse_args()
    from sketchyscenecolorization_amd import hip, matching
    if not torch.cuda.is_available():
        raise SystemExit('match_rate.py measures on the device: no GPU here')
    cfg = matching.MatchConfig(size=args.size)
    t0 = time.perf_counter()
    model = matching.MatchModel(cfg)
    model.init_random(1)
    torch.cuda.synchronize()
    load_s = time.perf_counter() - t0
    rng = np.random.RandomState(0)
    s = cfg.size
    sketch = np.full((s, s, 3), 255, np.uint8)
    sketch[rng.rand(s, s) < 0.1] = 0
    boxes, masks = [], []
    for _ in range(args.instances):
        y1, x1 = rng.randint(0, s - s // 3, 2)
        y2, x2 = y1 + rng.randint(s // 8, s // 3), x1 + rng.randint(s // 8, s // 3)
        boxes.append([y1, x1, y2, x2])
        masks.append((rng.rand(y2 - y1 + 1, x2 - x1 + 1) < 0.3).astype(np.uint8))
    boxes = np.array(boxes, np.int32)
    vocab = {w: k for k, w in enumerate(['<pad>', '<unk>'] + ['w%d' % k for k in range(cfg.vocab_size - 2)])}
    text = ' '.join('w%d' % k for k in range(args.words))
    indices, seq_len = matching.preprocess_sentence(text, vocab, cfg.max_len)
    buf, offsets = matching.pack_masks(boxes, masks, s)
    buf_d, boxes_d, off_d = torch.from_numpy(buf).cuda(), torch.from_numpy(boxes).cuda(), torch.from_numpy(offsets).cuda()
    counts = torch.empty((len(masks), 2), dtype=torch.int64, device='cuda')
    scene = {'sketch': sketch, 'boxes': boxes, 'masks': masks, 'class_ids': np.zeros(len(masks), np.int32)}
    stages = {'backbone': [], 'head': [], 'finish': []}
    whole = []
    for rep in range(args.warmup + args.reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        skd, tok, n = model.upload(sketch, indices, seq_len)
        x4, stroke = hip.match_preprocess_u8(skd, out=model._buf('x4', (1, s, s, 4)), stroke=model._buf('stroke', (s, s), torch.uint8))
        feat = model.backbone(x4)
        ev[1].record()
        pred = model.head(feat, tok, n)
        ev[2].record()
        up, predicts = hip.match_finish(pred, stroke, up=model._buf('up', (s, s)), predicts=model._buf('predicts', (s, s), torch.uint8))
        hip.instance_occupancy(predicts, buf_d, boxes_d, off_d, out=counts)
        ev[3].record()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        matched, scores, _ = matching.match_instances(model, scene, text, vocab)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        if rep >= args.warmup:
            for k, name in enumerate(('backbone', 'head', 'finish')):
                stages[name].append(ev[k].elapsed_time(ev[k + 1]))
            whole.append(wall * 1e3)
    med = {k: statistics.median(v) for k, v in stages.items()}
    lines = ['match_rate.py: one match at %d x %d, %d words, %d instances, random weights; medians of %d repetitions after %d warm-up '
             'passes, device events; %s, library %s' % (s, s, seq_len, len(masks), args.reps, args.warmup,
                                                        torch.cuda.get_device_name(0), hip.build_hash()),
             'load (host-made random weights, fold, pad, upload; wall clock, once)   %9.1f ms' % (load_s * 1e3),
             'backbone (input copy, preprocess, %d convs, max-pool, 4 rearrangements)   %9.3f ms  (min %.3f, max %.3f)'
             % (1 + sum(3 + (cin != cout) for _s, cin, cout, _st, _r in cfg.net.unit_list()), med['backbone'], min(stages['backbone']),
                max(stages['backbone'])),
             'head (projection, l2 norms, %d + %d LSTM steps, squash + projection)      %9.3f ms  (min %.3f, max %.3f)'
             % (seq_len, seq_len, med['head'], min(stages['head']), max(stages['head'])),
             'finish + selection (upsampling, threshold, %d instance counts)            %9.3f ms  (min %.3f, max %.3f)'
             % (len(masks), med['finish'], min(stages['finish']), max(stages['finish'])),
             'sum of the three stages                                                %9.3f ms' % sum(med.values()),
             'match_instances, wall clock (with mask upload and read-back)            %9.3f ms  (min %.3f, max %.3f)'
             % (statistics.median(whole), min(whole), max(whole)),
             'matched %d of %d instances.  Measured once on one box: a record, no comparison with anything earlier.' % (len(matched), len(masks))]
    print('\n'.join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    model.close()


if __name__ == '__main__':
    main()
