"""A scene coloured one instruction at a time, in one process (sketchyscene_colorization_main.py of the reference; DESIGN.md
section 8.14): the matcher, the instance generator and the background generator are loaded once, the scene's sketch, inner mask,
packed instance masks and the matcher's backbone features lie on the device from ``open`` on, and the current result stays there
as uint8 from one turn to the next.

    session = SceneSession(matcher, fg_trainer, bg_trainer, vocabs, data_base_dir, results_base_dir, scene_size)
    session.open(9996)
    session.color('the bus on the left is yellow')      # FG: MatchModel.predict on the kept features -> colorize_instances
    session.color('the sky is pink')                    # BG: colorize_background with the last processed background text
    session.withdraw()

A turn writes <id>_<k>.png, <id>_fg.png (BG turns), the report <id>_<k>.json and, last, the record (scene_records.py): a turn
that fails writes nothing.  The report's ``changed`` is ssc_scene_change_hist_u8 of the image before and after the turn."""
import json
import os
from types import SimpleNamespace

import numpy as np

from . import scene_records

PIXEL_LIMIT = 1 << 24           # what the turn report's kernel counts in one launch


def required_bytes(match_config, fg_block_type, fg_vocab_size, fg_image_size, bg_vocab_size, scene_size):
    """What a session allocates before its first forward pass, in bytes: {matcher, foreground, background, scene}.  The matcher's
    flat weight buffer and its backbone's scratch memory; the two trainers' parameter, gradient and optimizer buffers (a trainer
    has them whether it trains or not); the scene's images (sketch, current and new result, the marked instances), its inner mask
    and stroke map, the packed instance masks and the kept features.  The activations of a forward pass are allocated at first
    use and are not in the sum."""
    from . import matching, params
    stub = SimpleNamespace(cfg=match_config, cw=matching.pad32(match_config.w_rnn), cm=matching.pad32(match_config.m_rnn))
    weights = sum(-(-int(np.prod(shape)) // 64) * 64 for shape in matching.MatchModel._device_shapes(stub).values())
    s = int(scene_size)
    # four images, the inner mask and the stroke map, the packed masks (budgeted as two scenes' worth of bytes), the features
    scene = 4 * 3 * s * s + 2 * s * s + 2 * s * s + 4 * match_config.feat ** 2 * match_config.feat_channels
    return {'matcher': 4 * weights + int(match_config.net.scratch_bytes()),
            'foreground': params.store_bytes(fg_block_type, fg_vocab_size, fg_image_size, slots=3),
            'background': params.store_bytes('BG', bg_vocab_size, s, slots=4),
            'scene': scene}


def check_budget(need, free_bytes):
    """need: required_bytes' dict -> its sum.  ValueError naming the bytes when the sum is more than half of ``free_bytes``."""
    total = int(sum(need.values()))
    if 2 * total > int(free_bytes):
        raise ValueError('a scene session needs %d bytes on the device (%s) and would take more than half of the %d that are free'
                         % (total, ', '.join('%s %d' % kv for kv in sorted(need.items())), int(free_bytes)))
    return total


def changed_counts(hist):
    """int64 [256] of ssc_scene_change_hist_u8 -> the report's {"background": n, "instances": {"k": n, ...}} (non-zero ones)."""
    hist = [int(v) for v in np.asarray(hist).reshape(-1)]
    return {'background': hist[0], 'instances': {str(g - 1): hist[g] for g in range(1, 256) if hist[g] != 0}}


def _write_png(path, image):
    from PIL import Image
    Image.fromarray(image, 'RGB').save(path, 'PNG')


class SceneSession(object):
    """matcher: a MatchModel with its weights; fg_trainer: the GanTrainer of obj_lib/main_procedure.scene; bg_trainer: the
    BGTrainer of bg_colorization_main's scene mode; vocabs: {'match', 'fg', 'bg'} word -> index.  The matcher's and the background
    generator's size must be ``scene_size``.  noise_seed: as main_procedure.scene -- -1 draws on the device, n >= 0 gives the p-th
    matched instance of a turn torch.randn(1, 256, generator=torch.Generator().manual_seed(n + p)), in a session as in a fresh
    process."""

    def __init__(self, matcher, fg_trainer, bg_trainer, vocabs, data_base_dir, results_base_dir, scene_size, fg_max_len=15,
                 bg_max_len=8, color_gradient=True, noise_seed=-1):
        scene_size = int(scene_size)
        if scene_size < 16 or scene_size * scene_size > PIXEL_LIMIT:
            raise ValueError('scene_size %d: from 16 (the sky colour is sought in rows 5 and 6) to %d' % (scene_size, 1 << 12))
        if matcher.cfg.size != scene_size:
            raise ValueError('the matcher reads %d x %d sketches, the scene size is %d' % (matcher.cfg.size, matcher.cfg.size, scene_size))
        if not matcher.loaded:
            raise ValueError('the matcher has no weights: load_tf_checkpoint or init_random first')
        for name in ('match', 'fg', 'bg'):
            if not vocabs.get(name):
                raise ValueError('vocabs[%r] is missing: the %s vocabulary (word -> index)' % (name, name))
        self.matcher, self.fg, self.bg, self.vocabs = matcher, fg_trainer, bg_trainer, vocabs
        self.data_base_dir, self.results_base_dir, self.size = data_base_dir, results_base_dir, scene_size
        self.fg_max_len, self.bg_max_len = int(fg_max_len), int(bg_max_len)
        self.color_gradient, self.noise_seed = bool(color_gradient), int(noise_seed)
        self.image_id = self.scene = self.resident = self.current = None

    # ------------------------------------------------------------------ the scene
    def open(self, image_id):
        """Read the scene's files once, upload them once, run the matcher's backbone once; the current result is the last
        record's PNG, or the sketch."""
        import torch
        from . import fg_scene, matching
        from .bg_scene import grass_table
        scene = fg_scene.load_instances(self.data_base_dir, image_id, self.size)
        buf, offsets = matching.pack_masks(scene['boxes'], scene['masks'], self.size)
        dev = self.matcher.device
        masks_d = torch.from_numpy(buf).to(dev)
        views = [masks_d[int(o):int(o) + m.size].view(m.shape) for o, m in zip(offsets, scene['masks'])]
        self.resident = {'sketch': torch.from_numpy(scene['sketch']).to(dev), 'inner': torch.from_numpy(scene['inner']).to(dev),
                         'grass': torch.from_numpy(grass_table(scene['class_ids'])).to(dev), 'masks': views, 'packed': masks_d,
                         'boxes': torch.from_numpy(np.ascontiguousarray(scene['boxes'], dtype=np.int32).reshape(-1, 4)).to(dev),
                         'offsets': torch.from_numpy(offsets).to(dev), 'hist': torch.empty(256, dtype=torch.int64, device=dev)}
        self.feat, self.stroke = self.matcher.features(self.resident['sketch'])
        self.image_id, self.scene = str(scene['image_id']), scene
        self._reload()
        return self

    def _reload(self):
        """The current result from the last record's PNG, or from the sketch."""
        import torch
        from PIL import Image
        _new, last_name, _text, _records = scene_records.fetch(self.image_id, self.results_base_dir)
        if last_name == '':
            self.current = self.resident['sketch'].clone()
            return
        path = os.path.join(scene_records.results_dir(self.image_id, self.results_base_dir), last_name)
        image = np.array(Image.open(path).convert('RGB'), dtype=np.uint8)
        if image.shape != (self.size, self.size, 3):
            raise ValueError('%s is %d x %d, the scene size is %d' % (path, image.shape[0], image.shape[1], self.size))
        self.current = torch.from_numpy(np.ascontiguousarray(image)).to(self.matcher.device)

    def _opened(self):
        if self.scene is None:
            raise ValueError('no scene is open: SceneSession.open(image_id) first')

    # ------------------------------------------------------------------ a turn
    def match(self, text):
        """matching.match_instances' selection through the kept features: -> (matched indices, float64 occupancies)."""
        from . import hip, matching
        indices, seq_len = matching.preprocess_sentence(text, self.vocabs['match'], self.matcher.cfg.max_len)
        _up, predicts = self.matcher.predict(self.feat, self.stroke, indices, seq_len)
        r = self.resident
        counts = hip.instance_occupancy(predicts, r['packed'], r['boxes'], r['offsets']).cpu().numpy()
        if (counts < 0).any():
            raise RuntimeError('ssc_instance_occupancy refused instance %d' % int(np.nonzero(counts[:, 0] < 0)[0][0]))
        return matching.select_instances(counts)

    def color(self, text):
        """One instruction -> its report (a dict; also written as <id>_<k>.json).  ValueError, and nothing written, for an
        instruction the networks refuse; the session can go on with the next one."""
        import torch
        from . import bg_scene, fg_scene, hip
        self._opened()
        if text is None or text == '':
            raise ValueError('an instruction is needed')
        kind = scene_records.colorize_type(text)
        new_name, _last_name, last_bg_text, records = scene_records.fetch(self.image_id, self.results_base_dir)
        report = {'colorization_type': kind, 'input_text': text, 'result_name': new_name}
        marked_d = None
        if kind == 'FG':
            matched, scores = self.match(text)
            noise = None
            if self.noise_seed >= 0 and matched:
                noise = torch.cat([torch.randn(1, 256, generator=torch.Generator().manual_seed(self.noise_seed + p))
                                   for p in range(len(matched))])
            facts = {}
            result_d, processed = fg_scene.colorize_instances(self.fg, self.scene, text, matched, self.current, vocab=self.vocabs['fg'],
                                                              text_len=self.fg_max_len, noise=noise, info=facts,
                                                              resident=self.resident, on_device=True)
            proc_bg_text = last_bg_text
            report.update(processed_text=processed, matched_inst_indices=matched,
                          matched_classes=[int(i['class']) for i in facts['instances']],
                          roads=[i['road'] for i in facts['instances']])
        else:
            facts = {}
            result_d, marked_d, processed = bg_scene.colorize_background(self.bg, self.scene, text, self.current, last_bg_text,
                                                                         self.color_gradient, vocab=self.vocabs['bg'],
                                                                         text_len=self.bg_max_len, info=facts,
                                                                         resident=self.resident, on_device=True)
            proc_bg_text = processed
            report.update(processed_text=processed, matched_inst_indices=[], matched_classes=[],
                          color_gradient=int(self.color_gradient), sky_color=facts['sky_color'], sky_bottom=facts['sky_bottom'],
                          start_height=facts['start_height'])
        hist_d = hip.scene_change_hist_u8(self.current, result_d, self.resident['inner'], out=self.resident['hist'])
        result = result_d.cpu().numpy()
        report['changed'] = changed_counts(hist_d.cpu().numpy())
        k = len(records) + 1
        out_dir = scene_records.results_dir(self.image_id, self.results_base_dir)
        os.makedirs(out_dir, exist_ok=True)
        _write_png(os.path.join(out_dir, new_name), result)
        if marked_d is not None:
            _write_png(os.path.join(out_dir, self.image_id + '_fg.png'), marked_d.cpu().numpy())
        with open(os.path.join(out_dir, scene_records.report_name(self.image_id, k)), 'w') as fp:
            json.dump(report, fp, sort_keys=True)
            fp.write('\n')
        scene_records.append(self.image_id, text, self.results_base_dir, kind, new_name, proc_bg_text, records)
        self.current = result_d
        return report

    def withdraw(self):
        """Take the last instruction back: its record, PNG and report go, the current result is the one before it (or the
        sketch).  ValueError without a record.  -> the records that are left."""
        self._opened()
        left = scene_records.withdraw(self.image_id, self.results_base_dir)
        self._reload()
        return left

    def close(self):
        self.matcher.close()
