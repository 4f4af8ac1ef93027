#!/usr/bin/env python
"""What painting one instance into a user scene costs (obj_colorization_main.py --mode scene).

One process, a trainer with freshly initialised weights at the generator size 192 (the cost does not depend on them), and one
synthetic scene per --sizes entry (192 and 768): an instance whose box is a third of the scene, outlined, with strokes over it,
and a road of two bands.  After a warm-up instance, per repetition and between device events on the stream:

  mask, paste     hip.fg_scene_mask_u8, hip.fg_scene_paste_u8                        (new launches)
  road            hip.road_parallel_u8 on the road's 192 x 192 sketch                 (new launch)
  resize          resize_and_padding_mask_image_device, reverse_resize_image_device   (existing launches; their coefficient tables
                                                                                      are made on the host and uploaded inside)
  forward         GanTrainer.generate_u8, one instance
  overlay         hip.bg_scene_overlay_u8, once per scene
  host            the same instance by tests/fg_scene_oracle.py (NumPy + PIL: mask image, LANCZOS resize, the way back, paste,
                  overlay) given the generator's image, and the reference's road loop, wall clock

and a check that the device's bytes are the oracle's.  Writes --out (default profiles/fg_scene.txt)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np
import torch

S = 192


def synthetic_scene(size, rng):
    """Instance 0: a house whose box is a third of the scene; instance 1: a road of two bands across it."""
    boxes = np.array([[size // 8, size // 6, size // 8 + size // 3, size // 6 + size // 3 + 5],
                      [5 * size // 8, 2, 5 * size // 8 + size // 12, size - 2]], np.int32)
    inner = np.zeros((size, size), np.uint8)
    sketch = np.full((size, size, 3), 255, np.uint8)
    masks = []
    for k, (y1, x1, y2, x2) in enumerate(boxes.tolist()):
        bh, bw = y2 - y1, x2 - x1
        m = np.zeros((bh + 1, bw + 1), np.uint8)
        t = max(size // 192, 1)
        m[t:2 * t, :bw] = m[bh - 2 * t:bh - t, :bw] = 1
        if k == 0:
            m[:bh, t:2 * t] = m[:bh, bw - 2 * t:bw - t] = 1
            for _ in range(40):
                y, x = rng.randint(0, bh), rng.randint(0, bw)
                m[y, x:x + rng.randint(3, bw // 2)] = 1
        masks.append(m)
        inner[y1 + 1:y2 - 1, x1 + 1:x2 - 1] = k + 1
        sketch[y1:y2, x1:x2][m[:bh, :bw] == 1] = 0
    return {'image_id': 'synthetic', 'sketch': sketch, 'inner': inner, 'class_ids': np.array([15, 36], np.int32), 'boxes': boxes,
            'masks': masks}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--sizes', default='192,768')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--block_type', default='MRU', choices=['MRU', 'Pix2Pix', 'Residual'])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fg_scene.txt'))
    args = ap.parse_args()
    import fg_scene_oracle as O
    from sketchyscenecolorization_amd import fg_scene, hip
    from sketchyscenecolorization_amd.bg_scene import grass_table
    from sketchyscenecolorization_amd.obj_lib.input_pipeline import resize_and_padding_mask_image_device, reverse_resize_image_device
    from sketchyscenecolorization_amd.trainer import GanTrainer
    tr = GanTrainer(img=S, seed=1, block_type=args.block_type)
    tok = np.zeros((1, 15), np.int32)
    tok[0, :5] = (2, 3, 4, 5, 8)
    label = torch.tensor([fg_scene.CLASS_TO_COLOR_ID[15]], dtype=torch.int32, device='cuda')
    noise = torch.randn(1, 256, device='cuda')
    lines = ['fg_scene_rate.py: one instance per forward pass, generator %s at %d x %d, %d repetitions after a warm-up, %s, library %s'
             % (args.block_type, S, S, args.reps, torch.cuda.get_device_name(0), hip.build_hash())]
    for size in [int(v) for v in args.sizes.split(',')]:
        scene = synthetic_scene(size, np.random.RandomState(size))
        y1, x1, y2, x2 = scene['boxes'][0].tolist()
        bh, bw = y2 - y1, x2 - x1
        inner_d, sketch_d = torch.from_numpy(scene['inner']).cuda(), torch.from_numpy(scene['sketch']).cuda()
        grass_d = torch.from_numpy(grass_table(scene['class_ids'])).cuda()
        small_d, road_small_d = torch.from_numpy(scene['masks'][0]).cuda(), torch.from_numpy(scene['masks'][1]).cuda()
        road_sketch_d = resize_and_padding_mask_image_device(hip.fg_scene_mask_u8(road_small_d), S, 0)
        verdict = torch.empty(3, dtype=torch.int32, device='cuda')
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(9)]
        t = {k: [] for k in ('mask', 'resize in', 'forward', 'resize back', 'paste', 'overlay', 'road', 'chain wall', 'host', 'host road')}
        for rep in range(args.reps + 1):
            result_d = sketch_d.clone()
            torch.cuda.synchronize()
            w0 = time.perf_counter()
            ev[0].record()
            mask_d = hip.fg_scene_mask_u8(small_d)
            ev[1].record()
            sk_d = resize_and_padding_mask_image_device(mask_d, S, 10)
            ev[2].record()
            gen = tr.generate_u8(sk_d[None], tok, noise, labels=label)
            ev[3].record()
            inst_d = reverse_resize_image_device(gen[0], bh, bw, margin_size=10)
            ev[4].record()
            hip.fg_scene_paste_u8(result_d, inner_d, inst_d, y1, x1, 1)
            ev[5].record()
            hip.bg_scene_overlay_u8(result_d, inner_d, grass_d, sketch_d)
            ev[6].record()
            torch.cuda.synchronize()
            w1 = time.perf_counter()
            ev[7].record()
            hip.road_parallel_u8(road_sketch_d, 25, out=verdict)
            ev[8].record()
            torch.cuda.synchronize()
            gen_h = gen[0].cpu().numpy()
            h0 = time.perf_counter()
            want_sketch = O.instance_sketch(scene, 0, S)
            want = O.finish(scene, [0], [gen_h])
            h1 = time.perf_counter()
            road_sketch = O.instance_sketch(scene, 1, S)
            h2 = time.perf_counter()
            want_road = O.road_loop(road_sketch)
            h3 = time.perf_counter()
            assert np.array_equal(sk_d.cpu().numpy(), want_sketch) and np.array_equal(result_d.cpu().numpy(), want)
            assert np.array_equal(road_sketch_d.cpu().numpy(), road_sketch)
            assert verdict.cpu().tolist() == [int(want_road)] + list(O.road_counts(road_sketch))
            if rep:         # the first instance is the warm-up
                for i, k in enumerate(('mask', 'resize in', 'forward', 'resize back', 'paste', 'overlay')):
                    t[k].append(ev[i].elapsed_time(ev[i + 1]))
                t['road'].append(ev[7].elapsed_time(ev[8]))
                t['chain wall'].append((w1 - w0) * 1e3)
                t['host'].append((h1 - h0) * 1e3)
                t['host road'].append((h3 - h2) * 1e3)
        lines.append('')
        lines.append('scene %d x %d, box %d x %d (%d of its pixels pasted), road verdict %s; device bytes == oracle bytes in every repetition'
                     % (size, size, bh, bw, int((scene['inner'][y1:y2, x1:x2] == 1).sum()), verdict.cpu().tolist()))
        for name, k in (('mask image (new launch), device events', 'mask'),
                        ('paste (new launch), device events', 'paste'),
                        ('road test on the 192 x 192 sketch (new launch), device events', 'road'),
                        ('resize to the generator: LANCZOS, pad (2 existing launches + tables), device events', 'resize in'),
                        ('resize back to the box: bilinear (2 existing launches + tables), device events', 'resize back'),
                        ('forward pass (generate_u8, one instance), device events', 'forward'),
                        ('strokes over the scene (existing launch, once per scene), device events', 'overlay'),
                        ('the whole chain of one instance, launch to synchronise, wall clock', 'chain wall'),
                        ('the same instance without the forward pass by the NumPy + PIL oracle on the host, wall clock', 'host'),
                        ("the reference's road loop on the host, wall clock", 'host road')):
            v = np.array(t[k])
            lines.append('%-100s median %9.3f ms   min %9.3f   max %9.3f' % (name, np.median(v), v.min(), v.max()))
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fp:
        fp.write(text)
    print(text, end='')


if __name__ == '__main__':
    main()
