"""The instances of a user scene, as the scene pipeline colours them (Pipeline_utils/fg_color_utils.py::
build_instance_colorization): the instruction cut down to what the Foreground generator was trained on, and per named instance
its mask image cut from the segmentation data, the LANCZOS resize to the generator's size, one forward pass of its own, the
bilinear way back to the box and the masked paste into the scene; the sketch strokes go over the result at the end
(hip.fg_scene_mask_u8, road_parallel_u8, fg_scene_paste_u8, bg_scene_overlay_u8 and the two device resizes of
obj_lib/input_pipeline.py).

One instance per forward pass, in the order given, as the reference runs them (batch_size = 1, :202): the generators' norms are
batch statistics, so a batch of instances would give every one of them other pixels.  The reference's Instance_Matching step is
not here: the caller names the instances.  Matching, result records and ``withdraw`` are scene_session.SceneSession's, which
calls this with the scene and the previous result kept on the device (sketchyscene_colorization_main.py)."""
import os
import re

import numpy as np

from .bg_scene import grass_table, load_scene

ROAD_LABEL = 36
GRASS_LABEL = 27
# skeId_carId_map (:18-21): class of the 46-class segmentation -> the generator's class label
CLASS_TO_COLOR_ID = {7: 0, 9: 1, 12: 2, 13: 3, 14: 4, 15: 5, 16: 6, 17: 7, 18: 8, 19: 9, 22: 10, 23: 11, 27: 12, 28: 13, 29: 14,
                     30: 15, 32: 16, 34: 17, 35: 18, 36: 19, 37: 20, 39: 21, 41: 22, 43: 23, 44: 24}
PARALLEL_WIDTH = 25         # is_road_not_single_line's default
# Instance_Matching/data_processing/text_processing.py:26-39 (its es_attr list, :41, only feeds a plural flag that this path drops)
SIMPLE_COLORS = ['brown', 'gray', 'black', 'red', 'green', 'blue', 'yellow', 'orange', 'pink', 'purple', 'cyan', 'white']
CATEGORIES = ['bench', 'bird', 'bus', 'butterfly', 'car', 'cat', 'chair', 'chicken', 'cloud', 'cow', 'dog', 'duck', 'horse',
              'house', 'grass', 'moon', 'person', 'pig', 'rabbit', 'road', 'sheep', 'star', 'sun', 'tree', 'truck']
CATEGORIES_PLURAL = ['benches', 'birds', 'buses', 'butterflies', 'cars', 'cats', 'chairs', 'chickens', 'clouds', 'cows', 'dogs',
                     'ducks', 'horses', 'houses', 'grasses', 'moons', 'people', 'pigs', 'rabbits', 'roads', 'sheep', 'stars',
                     'suns', 'trees', 'trucks']
VERBS = ('has', 'have', 'is', 'are')
_SPLIT = re.compile(r'(\W+)')


def _words(text, keep_dash=True):
    return [w.lower() for w in _SPLIT.split(text.strip()) if len(w.strip()) > 0 and (keep_dash or w != '-')]


def self_category(text):
    """The first category word of the text, in the singular, or None (search_for_self_category)."""
    for w in _words(text, keep_dash=False):
        if w in CATEGORIES:
            return w
        if w in CATEGORIES_PLURAL:
            return CATEGORIES[CATEGORIES_PLURAL.index(w)]
    return None


def has_color(text):
    return any(w in SIMPLE_COLORS for w in _words(text, keep_dash=False))


def judging_preposition(text, verb):
    """False when the word 'with' stands in front of the word ``verb`` ('a man with blue pants has red shirt': the text must
    not be cut at the verb).  ValueError when 'with' is a word of the text and ``verb`` is not, where the reference dies."""
    words = _words(text)
    if 'with' in words:
        if verb.lower() not in words:
            raise ValueError("%r: %r is found inside another word only, and the text holds 'with': the reference cannot place "
                             "one against the other (list.index fails)" % (text, verb))
        if words.index('with') < words.index(verb.lower()):
            return False
    return True


def segment_user_input_text(text):
    """'the bus on the left is yellow with blue windows' -> 'the bus is yellow with blue windows' (:51-77): the text is cut at
    the first 'has', 'have', 'is' or 'are' -- tried in that order, found as a substring of the string, as the reference finds
    it -- that no 'with' precedes, and 'the <category>' is put in front of the verb's half when that half names a colour and
    the other does not.  Everything else comes back unchanged."""
    for verb in VERBS:
        if verb in text and judging_preposition(text, verb):
            at = text.index(verb)
            break
    else:
        return text
    head, tail = text[:at], text[at:]
    if has_color(head) or not has_color(tail):
        return text
    category = self_category(text)
    if category is None:
        raise ValueError('%r names no category the instruction could be rebuilt around' % text)
    return 'the ' + category + ' ' + tail


def load_instances(scene_dir, image_id, size):
    """bg_scene.load_scene's dict plus ``boxes`` int32 [N,4] = (y1, x1, y2, x2) and ``masks``, the list of the N small masks
    uint8 [y2-y1+1, x2-x1+1], from ``seg_data/<id>_datas.npz`` (keys pred_boxes, pred_masks).  ValueError for a mask of another
    shape and for a box that is empty or leaves the size x size image."""
    scene = load_scene(scene_dir, image_id, size)
    with np.load(os.path.join(scene_dir, 'seg_data', str(image_id) + '_datas.npz'), allow_pickle=True) as npz:
        boxes = np.array(npz['pred_boxes'], dtype=np.int32).reshape(-1, 4)
        masks = [np.ascontiguousarray(m, dtype=np.uint8) for m in npz['pred_masks']]
    check_instances(scene['image_id'], boxes, masks, scene['class_ids'], size, size)
    scene.update(boxes=boxes, masks=masks)
    return scene


def check_instances(image_id, boxes, masks, class_ids, h, w):
    if not (len(boxes) == len(masks) == len(np.asarray(class_ids).reshape(-1))):
        raise ValueError('scene %s: %d boxes, %d masks and %d classes' % (image_id, len(boxes), len(masks),
                                                                           len(np.asarray(class_ids).reshape(-1))))
    for k, ((y1, x1, y2, x2), m) in enumerate(zip(boxes.tolist(), masks)):
        if y1 < 0 or x1 < 0 or y2 - y1 < 1 or x2 - x1 < 1 or y2 > h or x2 > w:
            raise ValueError('scene %s: the box (%d, %d, %d, %d) of instance %d is empty or leaves the %d x %d image'
                             % (image_id, y1, x1, y2, x2, k, h, w))
        if m.shape != (y2 - y1 + 1, x2 - x1 + 1):
            raise ValueError('scene %s: the mask of instance %d is %s, its box (%d, %d, %d, %d) needs %s'
                             % (image_id, k, m.shape, y1, x1, y2, x2, (y2 - y1 + 1, x2 - x1 + 1)))


def _cut_is_empty(s, bh, bw, margin):
    """reverse_resize_image cuts round(s * (long - short) / long / 2) off both ends: nothing may be left of a thin box."""
    bh, bw = bh + 2 * margin, bw + 2 * margin
    return s - 2 * int(round(s * abs(bh - bw) / max(bh, bw) / 2.)) < 1


def colorize_instances(trainer, scene, text, inst_indices, previous_image=None, vocab=None, text_len=15, noise=None, info=None,
                       resident=None, on_device=False):
    """-> (result uint8 [H,W,3] on the host, processed text).

    trainer: a GanTrainer with the weights loaded (its image size S is the instances' size); scene: what load_instances returns;
    inst_indices: the instances to paint, each through a forward pass of its own, in this order; previous_image uint8 [H,W,3]
    defaults to the sketch; vocab: the caption vocabulary (word -> index); noise: float [len(inst_indices), 256] or None (drawn
    on the device, as inference mode draws it).  ``info`` (a dict) receives per instance the [S,S,3] sketch the generator read
    (before grass is thickened), the [S,S,3] image it made and, for a road, {V, Hc}.

    A scene session (scene_session.py) keeps the scene on the device between its turns: previous_image may be a uint8 [H,W,3]
    tensor on the device (it is copied, never written); ``resident``: a dict of device tensors that were uploaded once -- sketch
    uint8 [H,W,3], inner uint8 [H,W], grass uint8 [256] (grass_table) and masks, the list of the N small masks -- read in place
    of the uploads here; on_device: the result comes back as a device tensor and is not read.  The launches are the same.

    ValueError before any launch for an instance whose class the generator does not know, and after the last launch -- nothing
    is returned then -- for a road that is a single line.  The road verdicts stay on the device until the image is read."""
    import torch
    from . import hip
    from .data_processing.text_processing import preprocess_sentence
    from .obj_lib.input_pipeline import resize_and_padding_mask_image_device, reverse_resize_image_device
    if vocab is None:
        raise ValueError('colorize_instances needs the caption vocabulary (load_vocab_dict_from_file)')
    sketch, inner, class_ids = scene['sketch'], scene['inner'], np.asarray(scene['class_ids']).reshape(-1)
    boxes, masks = np.asarray(scene['boxes']), scene['masks']
    h, w = inner.shape
    s = int(trainer.img)
    inst_indices = [int(k) for k in inst_indices]
    if previous_image is None:
        previous_image = sketch
    previous_on_device = isinstance(previous_image, torch.Tensor)
    if previous_on_device:
        if previous_image.dtype != torch.uint8 or not previous_image.is_cuda or not previous_image.is_contiguous():
            raise ValueError('a previous image given as a tensor must be contiguous uint8 on the device')
    else:
        previous_image = np.ascontiguousarray(previous_image, dtype=np.uint8)
    if tuple(previous_image.shape) != (h, w, 3) or sketch.shape != (h, w, 3):
        raise ValueError('previous image %s and sketch %s must both be %d x %d x 3' % (tuple(previous_image.shape), sketch.shape, h, w))
    if noise is not None and tuple(noise.shape) != (len(inst_indices), 256):
        raise ValueError('noise is %s, %d instances need [%d, 256]' % (tuple(noise.shape), len(inst_indices), len(inst_indices)))
    check_instances(scene.get('image_id', '?'), boxes, masks, class_ids, h, w)
    for k in inst_indices:
        if not 0 <= k < min(len(class_ids), 255):
            raise ValueError('instance %d: the scene has instances 0..%d' % (k, min(len(class_ids), 255) - 1))
        if int(class_ids[k]) not in CLASS_TO_COLOR_ID:
            raise ValueError('instance %d has class %d, which the instance generator does not colour' % (k, int(class_ids[k])))
        y1, x1, y2, x2 = boxes[k].tolist()
        if _cut_is_empty(s, y2 - y1, x2 - x1, 0 if int(class_ids[k]) == ROAD_LABEL else 10):
            raise ValueError('instance %d: its %d x %d box is too thin to be cut back out of a %d x %d image'
                             % (k, y2 - y1, x2 - x1, s, s))
    processed = segment_user_input_text(text)
    tok = np.array(preprocess_sentence(processed, vocab, text_len), dtype=np.int32)[None]
    result_d = previous_image.clone() if previous_on_device else torch.from_numpy(previous_image).cuda()
    if resident is not None:
        inner_d, sketch_d, grass_d, masks_d = resident['inner'], resident['sketch'], resident['grass'], resident['masks']
    else:
        inner_d, sketch_d, grass_d, masks_d = torch.from_numpy(np.ascontiguousarray(inner)).cuda(), None, None, None
    if noise is not None:
        noise = torch.as_tensor(noise, dtype=torch.float32).cuda()
    roads = torch.ones((max(len(inst_indices), 1), 3), dtype=torch.int32, device='cuda')
    steps = []
    for p, k in enumerate(inst_indices):
        cls = int(class_ids[k])
        y1, x1, y2, x2 = boxes[k].tolist()
        bh, bw = y2 - y1, x2 - x1
        margin = 0 if cls == ROAD_LABEL else 10
        mask_d = hip.fg_scene_mask_u8(masks_d[k] if masks_d is not None else torch.from_numpy(masks[k]).cuda())
        if (bh, bw) != (s, s):
            sketch_k = resize_and_padding_mask_image_device(mask_d, s, margin)
        else:       # a box of the generator's size goes in as it is (:298-302): the channel is replicated, nothing more
            sketch_k = hip.resample_u8(mask_d, s, s, None, None, chan=0, out_channels=3)
        if cls == ROAD_LABEL:
            hip.road_parallel_u8(sketch_k, PARALLEL_WIDTH, out=roads[p])
        noise_k = noise[p:p + 1] if noise is not None else torch.randn(1, 256, device='cuda')
        label = torch.tensor([CLASS_TO_COLOR_ID[cls]], dtype=torch.int32, device='cuda')
        gen = trainer.generate_u8(sketch_k[None], tok, noise_k, labels=label, thicken=(cls == GRASS_LABEL))
        inst_d = reverse_resize_image_device(gen[0], bh, bw, margin_size=margin)
        hip.fg_scene_paste_u8(result_d, inner_d, inst_d, y1, x1, k + 1)
        steps.append((k, cls, sketch_k, gen))
    if resident is None:
        grass_d, sketch_d = torch.from_numpy(grass_table(class_ids)).cuda(), torch.from_numpy(sketch).cuda()
    hip.bg_scene_overlay_u8(result_d, inner_d, grass_d, sketch_d)
    result = result_d if on_device else result_d.cpu().numpy()
    verdicts = roads.cpu().numpy()      # read together: nothing came back before
    if info is not None:
        info['instances'] = [{'index': k, 'class': cls, 'sketch': sk.cpu().numpy(), 'generated': gen[0].cpu().numpy(),
                              'road': ({'V': int(verdicts[p, 1]), 'Hc': int(verdicts[p, 2])} if cls == ROAD_LABEL else None)}
                             for p, (k, cls, sk, gen) in enumerate(steps)]
    for p, (k, cls, _, _) in enumerate(steps):
        if cls == ROAD_LABEL and verdicts[p, 0] == 0:
            raise ValueError('instance %d: the road is a single line (%d columns and %d rows cross two strokes, %d are needed)'
                             % (k, int(verdicts[p, 1]), int(verdicts[p, 2]), PARALLEL_WIDTH))
    return result, processed
