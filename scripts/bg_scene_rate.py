#!/usr/bin/env python
"""What the finishing of a scene background costs at 768 x 768 (bg_colorization_main.py --mode scene).

One process, one synthetic scene (a sky band over a ground band, three instances of which one is grass, a few hundred strokes),
a trainer with freshly initialised weights (the cost does not depend on them).  After one warm-up scene, per repetition:

  forward    hip.bg_stage_u8 + G.forward, between two device events
  finishing  hip.bg_scene_crop_u8 + bg_scene_compose_u8 + bg_sky_gradient_u8 (3 launches) + bg_scene_overlay_u8, between two events
  host       the same finishing by tests/bg_scene_oracle.py (float64 NumPy) on the generator's image, wall clock

and a check that the device's bytes are the oracle's.  Writes --out (default profiles/bg_scene.txt)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np
import torch


def synthetic_scene(size, rng):
    inner = np.zeros((size, size), np.uint8)
    inner[size // 3:size // 2, size // 8:size // 3] = 1
    inner[3 * size // 4:, size // 4:] = 2
    inner[size // 8:size // 4, size // 2:3 * size // 4] = 3
    sketch = np.full((size, size, 3), 255, np.uint8)
    for _ in range(400):
        y, x = rng.randint(0, size, 2)
        n = rng.randint(5, 80)
        if rng.rand() < 0.5:
            sketch[y, x:x + n] = 0
        else:
            sketch[y:y + n, x] = 0
    return {'image_id': 'synthetic', 'sketch': sketch, 'inner': inner, 'class_ids': np.array([15, 27, 10], np.int32)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--size', type=int, default=768)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bg_scene.txt'))
    args = ap.parse_args()
    import bg_scene_oracle as O
    from sketchyscenecolorization_amd import bg_scene, hip
    from sketchyscenecolorization_amd.bg_colorization import BGTrainer
    size = args.size
    rng = np.random.RandomState(0)
    scene = synthetic_scene(size, rng)
    tr = BGTrainer(image_size=size, seed=1)
    # a previous result with a flat sky and ground, so that the gradient has a sky to find whatever the weights paint
    prev = np.empty((size, size, 3), np.uint8)
    prev[:size // 2], prev[size // 2:] = (90, 150, 230), (60, 160, 70)
    sketch_d, inner_d = torch.from_numpy(scene['sketch']).cuda(), torch.from_numpy(scene['inner']).cuda()
    grass_d, prev_d = torch.from_numpy(bg_scene.grass_table(scene['class_ids'])).cuda(), torch.from_numpy(prev).cuda()
    x = torch.empty((1, size, size, 3), dtype=torch.float32, device='cuda')
    y, xd, cnt = torch.empty_like(x), torch.empty((1, size, size, 8), dtype=torch.float32, device='cuda'), torch.empty(1, device='cuda')
    lab0 = torch.zeros((1, size, size), dtype=torch.int32, device='cuda')
    tok = np.zeros((1, 8), np.int32)
    tok[0, 2:] = (2, 3, 4, 5, 8, 7)
    # the image the finishing is timed on: the flat previous result as a float image (the untrained generator's output has no
    # most-frequent sky colour worth the name); the forward pass is timed on its own
    flat = (torch.from_numpy(prev).cuda().float() / 255.0 * 2.0 - 1.0).view(1, size, size, 3).contiguous()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    fwd, fin, host = [], [], []
    for rep in range(args.reps + 1):
        fg_d = hip.bg_scene_crop_u8(prev_d, inner_d)
        torch.cuda.synchronize()
        ev[0].record()
        fg4 = fg_d.view(1, size, size, 3)
        hip.bg_stage_u8(fg4, fg4, lab0, x, y, xd, cnt)
        tr.G.forward(x, tok, None, 'bg')
        ev[1].record()
        fg_d = hip.bg_scene_crop_u8(prev_d, inner_d)
        out_d, marked_d = hip.bg_scene_compose_u8(flat, fg_d, inner_d, grass_d, sketch_d)
        out_d, status_d, info_d = hip.bg_sky_gradient_u8(out_d, inner_d)
        hip.bg_scene_overlay_u8(out_d, inner_d, grass_d, sketch_d)
        ev[2].record()
        torch.cuda.synchronize()
        assert int(status_d.cpu()[0]) == 0
        img = flat.cpu().numpy()[0]
        t0 = time.perf_counter()
        want, want_marked, status, info = O.finish(img, prev, scene['inner'], scene['class_ids'], scene['sketch'], True)
        t1 = time.perf_counter()
        assert np.array_equal(out_d.cpu().numpy(), want) and np.array_equal(marked_d.cpu().numpy(), want_marked)
        if rep:         # the first scene is the warm-up
            fwd.append(ev[0].elapsed_time(ev[1]))
            fin.append(ev[1].elapsed_time(ev[2]))
            host.append((t1 - t0) * 1e3)
    lines = ['bg_scene_rate.py: one %d x %d scene, %d repetitions after a warm-up, %s, library %s'
             % (size, size, args.reps, torch.cuda.get_device_name(0), hip.build_hash()),
             'sky colour %s, sky_bottom %d, start_height %d; device bytes == oracle bytes in every repetition'
             % (info['sky_color'], info['sky_bottom'], info['start_height'])]
    for name, v in (('forward pass (stage + G.forward), device events', fwd),
                    ('finishing on the device (crop, compose, gradient x 3, overlay: 6 launches), device events', fin),
                    ('finishing by the float64 NumPy oracle on the host, wall clock', host)):
        v = np.array(v)
        lines.append('%-95s median %9.3f ms   min %9.3f   max %9.3f' % (name, np.median(v), v.min(), v.max()))
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fp:
        fp.write(text)
    print(text, end='')


if __name__ == '__main__':
    main()
