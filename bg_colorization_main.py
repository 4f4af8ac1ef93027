#!/usr/bin/env python
"""Command line of the Background_Colorization module on the MI355X-native HIP path.

Same flags and defaults as the reference (bg_colorization_main.py:978-1003), same run directory
``outputs/<UTC stamp>/{snapshot,log,results}``, snapshots named ``snapshot-<global step>``, test mode writing
``<bg name>_{inputs,outputs,targets}.png`` with the foreground pasted back over the generated background (:861-871).

Data layout under --data_base_dir (reference :739-750): ``foreground/<mode>/*.png``, ``background/<mode>/*.png``,
``segment/<mode>/*.png`` and ``captions/<mode>.json`` (records with fg_name, bg_name, color_text).  When the caption
file is missing the run uses seeded synthetic scenes, so the CLI can be exercised without the dataset.

--scene_cache device decodes every distinct training file once at start-up and keeps the scenes on the device as uint8; a step
then gathers its scenes by index inside the step's graph and no image is decoded or uploaded again.  The run is the one of
--scene_cache off, bit for bit.  --recolor 1 (with the cache) trains on the base records and paints sky and ground of every sample
with a freshly drawn colour pair, caption to match (class CachedScenes).  Both are off by default; test mode ignores them.

--batch_size N trains on N scenes per step (the reference's placeholders are fixed at 1, :765-768; nothing else in its graph
is): the norms' statistics, the loss means and the masked-L1 pixel count then run over the whole batch.  Test mode stays at
one image per forward pass, because those batch statistics would make every output depend on its batch mates.

--metrics 1 (test mode) scores every ``outputs`` image against its ``targets`` image on the device -- mean absolute error, PSNR
and SSIM (hip.image_metrics_u8) -- and writes ``results/metrics.json``.  Where the scene has a segment file its red channel is
the mask: the foreground pixels that were pasted back over the generation are not counted.

--val_freq F (train mode) scores a held-out set with the weights of the moment every F steps and on the last one: the scenes of
``foreground/val``, ``background/val``, ``segment/val`` and ``captions/val.json`` (the first --val_records of them), one per
forward pass, on the device.  A line per pass goes to ``log/validation.jsonl``: MAE / PSNR / SSIM as --metrics 1 defines them and
the region branch's pixel accuracy and IoU (sketchyscenecolorization_amd/bg_validation.py).  Training itself is the run of
--val_freq 0, bit for bit.  Without captions/val.json one line says so and the run trains on.

--color_metrics 1 adds colour scores where the two flags above score: CIELAB dE76 with its chroma and lightness parts, the
intersection of the ab histograms and colourfulness of output and target (hip.color_metrics_u8 / _bg_f32, under the same mask).
Test mode (with --metrics 1) also writes ``results/color_metrics.json``; train mode (with --val_freq F) adds the key "color" to
every line of ``log/validation.jsonl``.  It is refused where neither scores, and changes nothing when 0.

--mode scene --resume_from <stamp> --image_id <id> --instruction 'the sky is ...' colours the background of one user scene as the
reference's scene pipeline does (Pipeline_utils/bg_utils.py::build_background_colorization): ``<scene_dir>/sketches/<id>.png``,
``inner_masks/<id>.mat`` and ``seg_data/<id>_datas.npz`` are read, the instruction is spliced into --previous_text, the instances
of --previous_image (default: the sketch) go through one forward pass, and the device finishes the image -- instances and sketch
strokes pasted over the generation and, with --color_gradient 1, the sky gradient (sketchyscenecolorization_amd/bg_scene.py).
``outputs/<stamp>/scene_results/<id>/`` receives ``<id>_bg.png``, ``<id>_fg.png`` and ``scene.json``.  The caller keeps the
records: the next instruction names this result as --previous_image and the processed text as --previous_text.
"""
import argparse
import json
import os

os.environ.setdefault('HIP_FORCE_DEV_KERNARG', '1')     # kernel arguments in device memory (measured: 1570 vs 1540 images/s with 0)
import random
import time

import numpy as np
import torch

FLAGS = [
    ('mode', str, 'train', ['train', 'test', 'scene'], 'train, test, or scene: colour the background of one user scene'),
    ('resume_from', str, '', None, 'stamp of an earlier run under outputs/'),
    ('data_base_dir', str, 'data', None, 'dataset root'),
    ('image_size', int, 768, None, 'square image size'),
    ('batch_size', int, 1, None, 'scenes per training step; norm statistics and loss means run over the batch '
                                 '(test mode always feeds one image per pass: batch statistics would change every output)'),
    ('max_steps', int, 100000, None, 'training steps'),
    ('lr', float, 0.0002, None, 'initial Adam step size'),
    ('l1_weight', float, 100.0, None, 'weight of the masked L1 term'),
    ('gan_weight', float, 1.0, None, 'weight of the GAN term'),
    ('seg_weight', float, 100.0, None, 'weight of the region-mask term'),
    ('seg_classes', int, 3, None, 'region classes'),
    ('ngf', int, 64, None, 'generator width'),
    ('ndf', int, 64, None, 'discriminator width'),
    ('text_len', int, 8, None, 'caption length'),
    ('vocab_size', int, 18, None, 'caption vocabulary size'),
    ('vocab_file', str, 'data/bg_vocab.txt', None, 'vocabulary file'),
    ('summary_freq', int, 200, None, 'steps between scalar summaries'),
    ('progress_freq', int, 50, None, 'steps between progress prints'),
    ('save_freq', int, 20000, None, 'steps between snapshots (0 = never)'),
    ('scene_cache', str, 'off', ['off', 'device'], 'device: decode every distinct training file once at start-up and keep it '
                                                   'on the device as uint8; a step then gathers its scenes by index'),
    ('recolor', int, 0, [0, 1], '1 (needs --scene_cache device): train on the base records only and paint the sky and the ground '
                                'of every sample with a freshly drawn colour pair on the device, caption to match'),
    ('metrics', int, 0, [0, 1], '1 (--mode test): score every output against its target on the GPU (MAE, PSNR, SSIM; the '
                                'pasted-back foreground is not counted) and write results/metrics.json'),
    ('val_freq', int, 0, None, 'steps between held-out passes in train mode (0 = never): the scenes of {foreground,background,'
                               'segment}/val and captions/val.json are coloured one per pass with the current weights and scored '
                               'on the GPU (MAE, PSNR, SSIM; region accuracy and IoU) into log/validation.jsonl'),
    ('val_records', int, 0, None, 'held-out records a pass takes, the first ones in caption-file order (0 = all)'),
    ('val_preview', int, 0, None, 'every held-out pass (needs --val_freq F > 0) also writes log/previews/step_<n>.png and .json: a '
                                  'row for each of the first K scenes with its foreground, the output of the pass as --mode test '
                                  'would write it, and its background, made on the GPU; at most 32; 0 = none'),
    ('color_metrics', int, 0, [0, 1], '1: colour scores beside MAE / PSNR / SSIM, made on the GPU: CIELAB dE76, its chroma and '
                                      'lightness parts, the intersection of the ab histograms, colourfulness of output and target.  '
                                      '--mode test (needs --metrics 1) writes results/color_metrics.json; --mode train (needs '
                                      '--val_freq F > 0) adds a "color" key to every line of log/validation.jsonl'),
    ('scene_dir', str, 'examples', None, '--mode scene: directory with sketches/, inner_masks/ and seg_data/'),
    ('image_id', str, None, None, '--mode scene: the scene, <id> of sketches/<id>.png'),
    ('instruction', str, None, None, "--mode scene: what to paint, e.g. 'the sky is pink'"),
    ('previous_image', str, '', None, '--mode scene: the result of the last instruction, a png of the image size (default: the sketch)'),
    ('previous_text', str, '', None, "--mode scene: the processed text of the last instruction (default: 'the sky is blue and the "
                                     "ground is green')"),
    ('color_gradient', int, 1, [0, 1], '--mode scene: 1 = lighten the sky towards the top (add_color_gradient)'),
]
SCENE_FLAGS = ('scene_dir', 'image_id', 'instruction', 'previous_image', 'previous_text', 'color_gradient')


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    for name, typ, default, choices, text in FLAGS:
        parser.add_argument('--' + name, type=typ, default=default, choices=choices, help=text)
    return parser


class Scenes(object):
    """The four arrays of one training example: (inputs u8 [1,H,W,3], targets u8, token ids [1,T], labels [1,H,W])."""

    def __init__(self, p):
        self.p = p
        self.size, self.T = p['image_size'], p['text_len']
        base, mode = p['data_base_dir'], p['mode']
        self.dirs = {k: os.path.join(base, k, mode) for k in ('foreground', 'background', 'segment')}
        cap = os.path.join(base, 'captions', mode + '.json')
        self.records, self.vocab = None, None
        if os.path.exists(cap):
            from sketchyscenecolorization_amd.data_processing.text_processing import load_vocab_dict_from_file
            with open(cap) as fp:
                self.records = json.load(fp)
            self.vocab = load_vocab_dict_from_file(p['vocab_file'])
        print('## nImgs =', len(self), '\n')

    def __len__(self):
        return len(self.records) if self.records is not None else 8

    def get(self, idx, is_test=False):
        size = self.size
        if self.records is None:        # seeded synthetic scene
            rng = np.random.RandomState(1000 + idx)
            fg = np.full((1, size, size, 3), 255, np.uint8)
            fg[0, size // 4:size // 2, size // 4:size // 2] = rng.randint(0, 255, 3)
            bg = rng.randint(0, 255, (1, size, size, 3)).astype(np.uint8)
            lab = np.zeros((1, size, size), np.int32)
            lab[0, :size // 2] = 1
            lab[0, size // 2:] = 2
            lab[0, size // 4:size // 2, size // 4:size // 2] = 0
            tok = np.zeros((1, self.T), np.int32)
            tok[0, self.T - 4:] = rng.randint(1, self.p['vocab_size'], 4)
            return fg, bg, tok, (np.zeros_like(lab) if is_test else lab), 'synthetic_%d.png' % idx, 'synthetic_%d.png' % idx
        from sketchyscenecolorization_amd.data_processing.image_processing import load_image, load_region_mask
        from sketchyscenecolorization_amd.data_processing.text_processing import preprocess_sentence
        rec = self.records[idx]
        fg = load_image(os.path.join(self.dirs['foreground'], rec['fg_name']), size)
        bg = load_image(os.path.join(self.dirs['background'], rec['bg_name']), size)
        tok = np.array(preprocess_sentence(rec['color_text'], self.vocab, self.T), dtype=np.int32)[None]
        # segment png: 0 = foreground, 128 = sky (1), 255 = ground (2)   (image_processing.py:14-24)
        lab = load_region_mask(os.path.join(self.dirs['segment'], rec['fg_name']), size, is_test)
        return fg, bg, tok, lab, rec['fg_name'], rec['bg_name']


class CachedScenes(object):
    """What --scene_cache device trains from: every distinct file decoded once into a SceneCache on the trainer's device, the
    captions tokenised once; a step is ``batch_size`` scene indices -> their cache entries and token ids.

    --recolor 1: the scenes are the base records (bg_name == fg_name: 'blue' sky over 'green' ground).  Every sample gets a
    (sky, ground) pair of its own, drawn uniformly from bg_palette.PAIRS (the 50 pairs with sky != ground, sky-major in the
    order of the reference's two colour lists) by a random.Random seeded with one random.randint here -- the scene draws of the
    steps are the ones of a run without recolouring.  The stage kernel paints the pair over the base background's sky and
    ground pixels, which is the reference's offline augmentation (data_preparation/bg_data_generation.py:139-160) with a fresh
    pair per sample instead of aug_num frozen ones per scene; the caption is that script's, for the drawn pair."""

    def __init__(self, p, scenes, device):
        from sketchyscenecolorization_amd.scene_cache import SceneCache
        keep, self.pair_rng = None, None
        if p.get('recolor', 0):
            from sketchyscenecolorization_amd.data_processing import bg_palette
            from sketchyscenecolorization_amd.data_processing.text_processing import preprocess_sentence
            if scenes.records is None:
                raise ValueError('--recolor 1 needs a dataset with a caption file: the synthetic scenes have no base records')
            keep = [i for i, r in enumerate(scenes.records) if r['bg_name'] == r['fg_name']]
            if not keep:
                raise ValueError('--recolor 1: none of the %d records is a base record (bg_name == fg_name) to recolour'
                                 % len(scenes.records))
            self.pair_rng = random.Random(random.randint(0, 2 ** 31 - 1))
            self.pair_tokens = np.array([preprocess_sentence(bg_palette.caption(s, g), scenes.vocab, scenes.T)
                                         for s, g in bg_palette.PAIRS], np.int32)
            self.pair_records = np.stack([bg_palette.recolor_record(s, g) for s, g in bg_palette.PAIRS])
        self.cache = SceneCache(scenes, device, keep)
        c = self.cache
        print('scene cache: %d scenes from %d foregrounds, %d backgrounds, %d segment maps; %.1f MB on %s, built in %.1f s'
              % (len(c), c.fg.shape[0], c.bg.shape[0], c.seg.shape[0], c.nbytes / 1e6, c.device, c.build_seconds))

    def __len__(self):
        return len(self.cache)

    def step(self, tr, idxs):
        slots, tok, rec = self.cache.slots[idxs], self.cache.tokens[idxs], None
        if self.pair_rng is not None:
            pairs = [self.pair_rng.randint(0, len(self.pair_records) - 1) for _ in idxs]
            rec, tok = self.pair_records[pairs], self.pair_tokens[pairs]
        tr.train_step_cached(self.cache, slots, rec, tok)


def to_unit(u8):
    """uint8 [0,255] -> float [-1,1] (convert_image_dtype + preprocess, :30-33, 100-113) in torch arithmetic: what float callers
    of BGTrainer.train_step feed it with.  The command line itself stages its uint8 arrays with hip.bg_stage_u8."""
    u8 = u8 if torch.is_tensor(u8) else torch.from_numpy(u8)
    x = u8.to('cuda', torch.float32)
    # the divisor is a (0-dim) device tensor: torch turns a division by a Python number into a multiplication by its rounded
    # reciprocal, which is one ulp away from x / 255 for 111 of the 256 byte values
    return x / torch.full((), 255.0, dtype=torch.float32, device=x.device) * 2.0 - 1.0


def to_u8(x):
    """[-1,1] -> uint8 with saturation (deprocess + convert_image_dtype(saturate=True), :36-39, 785-786) in torch arithmetic;
    the command line's test mode runs the same operations in hip.bg_finish_u8."""
    y = ((x + 1.0) / 2.0).clamp(0.0, 1.0) * 255.0
    return (y + 0.5).floor().clamp(0, 255).to(torch.uint8).cpu().numpy()


def load_checkpoint(tr, snap_dir):
    """Load the snapshot that ``snap_dir/checkpoint`` names -- a tf.train.Saver bundle or a snapshot of this command line --
    into the trainer -> the global step it was taken at."""
    idx = os.path.join(snap_dir, 'checkpoint')
    with open(idx) as fp:
        name = fp.readline().split('"')[1]
    print('loading model from checkpoint', os.path.join(snap_dir, name))
    from sketchyscenecolorization_amd import tf_checkpoint
    if tf_checkpoint.is_tf_checkpoint(os.path.join(snap_dir, name)):    # a tf.train.Saver checkpoint (released model)
        tr.store.load_dict(tf_checkpoint.read_checkpoint(os.path.join(snap_dir, name)))
    else:
        sd = torch.load(os.path.join(snap_dir, name), map_location='cpu')
        tr.store.load_state_dict(sd)
        for sc in (tr.store.generator, tr.store.discriminator):
            if '__adam_m__/' + sc.name in sd:
                sc.adam_m.copy_(sd['__adam_m__/' + sc.name])
    tr.global_step = int(name.split('-')[1])
    return tr.global_step


def new_trainer(p):
    from sketchyscenecolorization_amd.bg_colorization import BGTrainer
    tr = BGTrainer(image_size=p['image_size'], vocab_size=p['vocab_size'], ngf=p['ngf'], ndf=p['ndf'],
                   seg_classes=p['seg_classes'], lr=p['lr'], max_steps=p['max_steps'], gan_weight=p['gan_weight'],
                   l1_weight=p['l1_weight'], seg_weight=p['seg_weight'], seed=random.randint(0, 2 ** 31 - 1))
    print('parameter_count =', tr.store.parameter_count('generator') + tr.store.parameter_count('discriminator'))
    return tr


def color_scene(p):
    """--mode scene: one instruction on one scene -> the directory the three files went to."""
    from PIL import Image
    from sketchyscenecolorization_amd import bg_scene
    from sketchyscenecolorization_amd.data_processing.text_processing import load_vocab_dict_from_file
    out_dir = os.path.join('outputs', p['resume_from'])
    scene = bg_scene.load_scene(p['scene_dir'], p['image_id'], p['image_size'])
    previous = None
    if p['previous_image'] != '':
        previous = np.array(Image.open(p['previous_image']).convert('RGB'), dtype=np.uint8)
        if previous.shape[:2] != (p['image_size'], p['image_size']):
            raise ValueError('--previous_image %s is %d x %d, --image_size is %d'
                             % (p['previous_image'], previous.shape[0], previous.shape[1], p['image_size']))
    vocab = load_vocab_dict_from_file(p['vocab_file'])
    tr = new_trainer(p)
    print('iter_from', load_checkpoint(tr, os.path.join(out_dir, 'snapshot')))
    facts = {}
    bg, fg, text = bg_scene.colorize_background(tr, scene, p['instruction'], previous, p['previous_text'], bool(p['color_gradient']),
                                                vocab=vocab, text_len=p['text_len'], info=facts)
    print('proc_input_text:', text)
    res_dir = os.path.join(out_dir, 'scene_results', scene['image_id'])
    os.makedirs(res_dir, exist_ok=True)
    Image.fromarray(bg, 'RGB').save(os.path.join(res_dir, scene['image_id'] + '_bg.png'), 'PNG')
    Image.fromarray(fg, 'RGB').save(os.path.join(res_dir, scene['image_id'] + '_fg.png'), 'PNG')
    with open(os.path.join(res_dir, 'scene.json'), 'w') as fp:
        json.dump(dict(facts, text=text, color_gradient=int(bool(p['color_gradient']))), fp, sort_keys=True)
        fp.write('\n')
    return res_dir


def bg_colorization(**p):
    if p['mode'] == 'scene':
        return color_scene(p)
    mode, stamp = p['mode'], p['resume_from']
    if stamp == '':
        if mode == 'test':
            raise Exception('checkpoint required for test mode')
        stamp = time.strftime('%Y-%m-%d-%H-%M-%S', time.gmtime())
    out_dir = os.path.join('outputs', stamp)
    snap_dir = os.path.join(out_dir, 'snapshot')
    os.makedirs(snap_dir, exist_ok=True)
    scenes = Scenes(p)
    tr = new_trainer(p)
    iter_from = load_checkpoint(tr, snap_dir) if p['resume_from'] != '' else 0
    print('iter_from', iter_from)

    if mode == 'test':
        from PIL import Image
        res_dir = os.path.join(out_dir, 'results')
        os.makedirs(res_dir, exist_ok=True)
        from sketchyscenecolorization_amd import hip
        size = p['image_size']
        names, rows, color_rows = [], [], []
        # one image per forward pass whatever --batch_size says: the norms are batch statistics
        for i in range(len(scenes)):
            print('Processing', i, '/', len(scenes))
            fg, bg, tok, lab, fg_name, bg_name = scenes.get(i, is_test=True)
            fg_d = torch.from_numpy(fg).cuda()
            gctx = tr.color_foreground(fg_d, tok)       # nothing but the foreground is uploaded
            seg_path = os.path.join(scenes.dirs['segment'], fg_name)
            inner = None
            if os.path.exists(seg_path):        # paste the foreground (segment value 0) back over the generation
                inner = torch.from_numpy(np.ascontiguousarray(np.array(Image.open(seg_path).convert('RGB'), np.uint8)[:, :, 0])).cuda()
            out_d = hip.bg_finish_u8(gctx['image'], fg_d, inner)
            out = out_d.cpu().numpy()
            if p.get('metrics', 0):     # out_d holds the bytes that are written below; the mask is the paste-back's
                bg_d, mask_d = torch.from_numpy(bg).cuda(), None if inner is None else inner.reshape(1, size, size)
                rows.append(hip.image_metrics_u8(out_d, bg_d, mask_d).cpu().numpy())
                if p.get('color_metrics', 0):
                    color_rows.append(hip.color_metrics_u8(out_d, bg_d, mask_d).cpu().numpy())
                names.append(bg_name[:-4])
            for kind, arr in (('inputs', fg), ('outputs', out), ('targets', bg)):
                Image.fromarray(arr[0], 'RGB').save(os.path.join(res_dir, bg_name[:-4] + '_' + kind + '.png'), 'PNG')
        if p.get('metrics', 0):
            from sketchyscenecolorization_amd import metrics as M
            summary = M.summarise(names, ['all'] * len(names), np.concatenate(rows, 0))
            with open(os.path.join(res_dir, 'metrics.json'), 'w') as fp:
                fp.write(M.dumps(summary))
            print(M.all_line(summary))
            if p.get('color_metrics', 0):
                csum = M.summarise_color(names, ['all'] * len(names), np.concatenate(color_rows, 0))
                with open(os.path.join(res_dir, 'color_metrics.json'), 'w') as fp:
                    fp.write(M.dumps(csum))
                print(M.color_line(csum))
        return

    log_dir = os.path.join(out_dir, 'log')
    os.makedirs(log_dir, exist_ok=True)
    start = time.time()
    ema = None
    # The examples of the next steps are loaded ahead (two 768 x 768 images and a region mask per scene: ~60 ms of decoding on
    # one thread against a 22 ms device step) by a few threads, in the order the indices are drawn -- batch_size draws per step,
    # one random.randint each, so the sequence at batch 1 is the one of one draw per step; SSC_BG_PREFETCH=0: loaded where they
    # are used.
    import collections
    from concurrent.futures import ThreadPoolExecutor
    nb = p['batch_size']
    cache = CachedScenes(p, scenes, tr.losses.device) if p.get('scene_cache', 'off') == 'device' else None
    n_scenes = len(cache) if cache is not None else len(scenes)
    held = None
    if p.get('val_freq', 0):        # the held-out set on the device, whatever --scene_cache says; both caches share one limit
        from sketchyscenecolorization_amd import bg_validation
        held = bg_validation.open_held_out(p, Scenes, tr, cache.cache.nbytes if cache is not None else 0)
    depth = int(os.environ.get('SSC_BG_PREFETCH', '4'))
    pool = ThreadPoolExecutor(max_workers=max(depth, 1) * min(nb, 4)) if depth > 0 and cache is None else None
    ahead, drawn = collections.deque(), [iter_from]

    def draw_batch():
        return [random.randint(0, n_scenes - 1) for _ in range(nb)]

    def draw_more():
        while pool is not None and len(ahead) < depth and drawn[0] < p['max_steps']:
            ahead.append([pool.submit(scenes.get, i) for i in draw_batch()])
            drawn[0] += 1

    # the scenes of a step are stacked into pinned staging buffers of the batch shape, allocated once and used in turn (pinning
    # a fresh 1.7 MB array costs 3.5 ms a time; a copy from pageable memory returns only when it has happened, behind the step
    # that is running).  A buffer is written again only when the copy that last read it has happened (pinned_ring.py).
    from sketchyscenecolorization_amd.pinned_ring import PinnedRing
    rings = []      # of the foreground, the background and the labels: made at the first step, of the shapes it loads

    for step in range(iter_from, p['max_steps']):
        def should(freq):
            return freq > 0 and ((step + 1) % freq == 0 or step == p['max_steps'] - 1)
        if cache is not None:       # the scenes are on the device: a step uploads their entries (and colour pairs) only
            cache.step(tr, draw_batch())
        elif pool is not None:
            draw_more()
            batch = [f.result() for f in ahead.popleft()]
            draw_more()
        else:
            batch = [scenes.get(i) for i in draw_batch()]
        if cache is None:
            if not rings:
                rings = [PinnedRing((nb,) + tuple(batch[0][k].shape[1:]), dt) for k, dt in ((0, torch.uint8), (1, torch.uint8), (3, torch.int32))]
            fg, bg, lab = [ring.next() for ring in rings]
            for k, buf in zip((0, 1, 3), (fg, bg, lab)):        # what Scenes.get returns: fg, bg, tokens, labels, names
                view = buf.numpy()
                for i, b in enumerate(batch):
                    view[i] = b[k][0]
            tr.train_step_u8(fg, bg, np.concatenate([b[2] for b in batch], 0), lab)
            for ring in rings:
                ring.queued()
        if should(p['progress_freq']) or should(p['summary_freq']):
            vals = tr.loss_values()
            # tf.train.ExponentialMovingAverage(0.99) of the five losses (:657-658), updated when they are read
            ema = list(vals) if ema is None else [0.99 * e + 0.01 * v for e, v in zip(ema, vals)]
            names = ('discrim_loss', 'gen_loss', 'gen_loss_GAN', 'gen_loss_L1', 'region_mask_loss')
            if should(p['summary_freq']):
                with open(os.path.join(log_dir, 'scalars.jsonl'), 'a') as fp:
                    fp.write(json.dumps(dict(zip(names, ema), step=tr.global_step)) + '\n')
            if should(p['progress_freq']):
                rate = (step - iter_from + 1) * p['batch_size'] / (time.time() - start)
                left = (p['max_steps'] - step) * p['batch_size'] / rate
                print('progress step %d  image/sec %0.1f  left time:%dd %dh %dm'
                      % (tr.global_step, rate, left // 86400, left % 86400 // 3600, left % 3600 // 60))
                for n, v in zip(names, ema):
                    print(n, v)
        if held is not None and should(p['val_freq']):
            bg_validation.run_pass(held, tr, log_dir)       # (reads the pending losses first, as a snapshot step settles them)
        if should(p['save_freq']):
            print('saving model to', snap_dir)
            name = 'snapshot-%d' % tr.global_step
            sd = tr.store.state_dict()
            for sc in (tr.store.generator, tr.store.discriminator):
                sd['__adam_m__/' + sc.name] = sc.adam_m.detach().cpu()
            torch.save(sd, os.path.join(snap_dir, name))
            with open(os.path.join(snap_dir, 'checkpoint'), 'w') as fp:
                fp.write('model_checkpoint_path: "%s"\n' % name)


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.mode == 'test':
        assert args.resume_from != ''
    if args.batch_size < 1:
        raise ValueError('--batch_size %d: at least one scene per step' % args.batch_size)
    if args.recolor and args.scene_cache != 'device':
        raise ValueError('--recolor 1 paints the cached scenes on the device: it needs --scene_cache device')
    if args.metrics and args.mode != 'test':
        raise ValueError('--metrics 1 scores the images of --mode test: training writes none')
    if args.val_freq < 0 or args.val_records < 0:
        raise ValueError('--val_freq %d --val_records %d: neither can be negative' % (args.val_freq, args.val_records))
    if args.val_freq and args.mode != 'train':
        raise ValueError('--val_freq %d scores a held-out set during --mode train: test mode scores its own images with --metrics 1'
                         % args.val_freq)
    from sketchyscenecolorization_amd import preview
    preview.checked_count(args.val_preview, args.val_freq, args.mode)
    from sketchyscenecolorization_amd import metrics
    metrics.checked_color_flag(args.color_metrics, args.metrics, args.val_freq, args.mode)
    defaults ={name: default for name, _t, default, _c, _h in FLAGS}
    if args.mode == 'scene':
        if args.resume_from == '':
            raise ValueError('--mode scene needs --resume_from <stamp>: the run whose snapshot colours the scene')
        if args.image_id is None or args.instruction is None:
            raise ValueError("--mode scene needs --image_id <id> and --instruction '<text>'")
        if args.image_size < 16:
            raise ValueError('--image_size %d: a scene is at least 16 x 16 (the sky colour is sought in rows 5 and 6 of the upper half)'
                             % args.image_size)
    else:
        given = [name for name in SCENE_FLAGS if getattr(args, name) != defaults[name]]
        if given:
            raise ValueError('--%s belongs to --mode scene, this is --mode %s' % (', --'.join(given), args.mode))
    bg_colorization(**{name: getattr(args, name) for name, _t, _d, _c, _h in FLAGS})


if __name__ == '__main__':
    main()
