"""The background of a user scene, as the scene pipeline colours it (Pipeline_utils/bg_utils.py::build_background_colorization):
the instruction spliced into the previous one, the previous result cropped to its instances, one forward pass of the Background
generator, and the finishing on the device -- instances and sketch strokes over the generation, the sky gradient, the strokes
once more (hip.bg_scene_crop_u8, bg_scene_compose_u8, bg_sky_gradient_u8, bg_scene_overlay_u8).

The caller hands the previous image and text in and keeps what comes back.  The reference's result records and ``withdraw``
(customization_util.py) are scene_records.py; scene_session.SceneSession keeps them, and the previous image on the device,
from one instruction to the next (sketchyscene_colorization_main.py)."""
import os
import re

import numpy as np

GRASS_LABEL = 27
DEFAULT_PREVIOUS_TEXT = 'the sky is blue and the ground is green'       # bg_utils.py:201-204
ALL_COLOR = ['blue', 'green', 'cyan', 'red', 'orange', 'yellow', 'brown', 'purple', 'pink', 'black', 'gray']
TEXT_TYPES = ['None', 'ground', 'sky', 'both']
SEARCH_FROM, SEARCH_HEIGHT = 5, 2       # add_color_gradient's defaults: the sky colour is sought in rows 5 and 6
_SPLIT = re.compile(r'(\W+)')


def _words(text):
    return [w.lower() for w in _SPLIT.split(text.strip()) if len(w.strip()) > 0]


def text_type(text):
    """'None', 'ground', 'sky' or 'both': which halves of a background instruction the text names (get_text_type, :24-37)."""
    words = _words(text)
    sky = 'sky' in words
    ground = 'ground' in words or 'floor' in words or 'land' in words
    return TEXT_TYPES[2 * sky + ground]


def _check_duplicated_color(text):
    sky, ground = '', ''
    for word in _words(text):
        if word in ALL_COLOR:
            if sky == '':
                sky = word
            else:
                ground = word
                break
    if sky == ground:       # two colourless halves are equal too, as in the reference
        raise ValueError('%r: the sky and the ground need two different colours (found %r and %r)' % (text, sky, ground))


def combine_text(new, previous):
    """The instruction the generator reads: ``new`` when it names sky and ground, otherwise ``new`` with the missing half taken
    from ``previous``, cut at its first 'and' (combine_bg_input_text, :59-93).  ValueError when ``new`` names neither, when
    ``previous`` lacks the missing half, or when both halves end up with the same colour."""
    kind, before = text_type(new), text_type(previous)
    if kind == 'None':
        raise ValueError('%r names neither the sky nor the ground' % new)
    if kind == 'both':
        out = new
    elif kind == 'sky':
        if before in ('None', 'sky'):
            raise ValueError('%r says nothing about the ground, and neither does the previous text %r' % (new, previous))
        if before == 'ground':
            out = new + ' and ' + previous
        else:
            if 'and' not in previous:
                raise ValueError("the previous text %r names sky and ground without an 'and' to cut it at" % previous)
            out = new + ' ' + previous[previous.index('and'):]
    else:
        if before in ('None', 'ground'):
            raise ValueError('%r says nothing about the sky, and neither does the previous text %r' % (new, previous))
        if before == 'sky':
            out = previous + ' and ' + new
        else:
            if 'and' not in previous:
                raise ValueError("the previous text %r names sky and ground without an 'and' to cut it at" % previous)
            out = previous[:previous.index('and')] + 'and ' + new
    _check_duplicated_color(out)
    return out


def grass_table(class_ids):
    """uint8 [256] indexed by the instance mask's value: 1 at k + 1 when instance k is grass (class 27), 0 at 0."""
    table = np.zeros(256, np.uint8)
    for k, c in enumerate(np.asarray(class_ids).reshape(-1)[:255]):
        if int(c) == GRASS_LABEL:
            table[k + 1] = 1
    return table


def load_scene(scene_dir, image_id, size):
    """``sketches/<id>.png`` (RGB, nearest-neighbour to size x size), ``inner_masks/<id>.mat`` (key inner_masks: 0 = background,
    k + 1 = instance k) and ``seg_data/<id>_datas.npz`` (key pred_class_ids) -> dict(image_id, sketch uint8 [size,size,3],
    inner uint8 [size,size], class_ids int [N])."""
    import scipy.io
    from PIL import Image
    image_id = str(image_id)
    sketch = Image.open(os.path.join(scene_dir, 'sketches', image_id + '.png')).convert('RGB')
    sketch = np.array(sketch.resize((size, size), resample=Image.NEAREST), dtype=np.uint8)
    inner = np.asarray(scipy.io.loadmat(os.path.join(scene_dir, 'inner_masks', image_id + '.mat'))['inner_masks'])
    if inner.shape != (size, size):
        raise ValueError('inner mask of scene %s is %s, the image size is %d x %d' % (image_id, inner.shape, size, size))
    if inner.min() < 0 or inner.max() > 255:
        raise ValueError('inner mask of scene %s holds values outside 0..255' % image_id)
    with np.load(os.path.join(scene_dir, 'seg_data', image_id + '_datas.npz')) as npz:
        class_ids = np.array(npz['pred_class_ids'])
    return {'image_id': image_id, 'sketch': np.ascontiguousarray(sketch), 'inner': np.ascontiguousarray(inner.astype(np.uint8)),
            'class_ids': class_ids}


STATUS_TEXT = {1: 'no background pixel (inner mask 0) in rows %d..%d, where the sky colour is sought'
                  % (SEARCH_FROM, SEARCH_FROM + SEARCH_HEIGHT - 1),
               2: 'the sky ends in the first rows (start_height 0): there is no height to spread the gradient over'}


def colorize_background(trainer, scene, text, previous_image=None, previous_text='', color_gradient=True, vocab=None,
                        text_len=8, info=None, resident=None, on_device=False):
    """-> (background uint8 [H,W,3], fg_marked uint8 [H,W,3], processed text), the arrays on the host.

    trainer: a BGTrainer with the weights loaded; scene: what load_scene returns; previous_image uint8 [H,W,3] defaults to the
    sketch and previous_text to 'the sky is blue and the ground is green'; vocab: the caption vocabulary (word -> index).
    The forward pass is test mode's: one image, zero labels.  ``info`` (a dict) receives sky_color, sky_bottom and start_height
    of the gradient (None without it).  ValueError for a text that cannot be combined and for a scene the gradient has no
    answer for.

    A scene session (scene_session.py) keeps the scene on the device between its turns: previous_image may be a uint8 [H,W,3]
    tensor on the device (it is read, never written); ``resident``: a dict of device tensors that were uploaded once -- sketch
    uint8 [H,W,3], inner uint8 [H,W] and grass uint8 [256] (grass_table) -- read in place of the uploads here; on_device: the
    two images come back as device tensors and are not read.  The launches are the same."""
    import torch
    from . import hip
    from .data_processing.text_processing import preprocess_sentence
    if vocab is None:
        raise ValueError('colorize_background needs the caption vocabulary (load_vocab_dict_from_file)')
    sketch, inner = scene['sketch'], scene['inner']
    h, w = inner.shape
    if previous_image is None:
        previous_image = sketch
    if previous_text == '':
        previous_text = DEFAULT_PREVIOUS_TEXT
    previous_on_device = isinstance(previous_image, torch.Tensor)
    if previous_on_device:
        if previous_image.dtype != torch.uint8 or not previous_image.is_cuda or not previous_image.is_contiguous():
            raise ValueError('a previous image given as a tensor must be contiguous uint8 on the device')
    else:
        previous_image = np.ascontiguousarray(previous_image, dtype=np.uint8)
    if tuple(previous_image.shape) != (h, w, 3) or sketch.shape != (h, w, 3):
        raise ValueError('previous image %s and sketch %s must both be %d x %d x 3' % (tuple(previous_image.shape), sketch.shape, h, w))
    processed = combine_text(text, previous_text)
    tok = np.array(preprocess_sentence(processed, vocab, text_len), dtype=np.int32)[None]
    if resident is not None:
        sketch_d, inner_d, grass_d = resident['sketch'], resident['inner'], resident['grass']
    else:
        sketch_d, inner_d = torch.from_numpy(sketch).cuda(), torch.from_numpy(inner).cuda()
        grass_d = torch.from_numpy(grass_table(scene['class_ids'])).cuda()
    fg_d = hip.bg_scene_crop_u8(previous_image if previous_on_device else torch.from_numpy(previous_image).cuda(), inner_d)
    gctx = trainer.color_foreground(fg_d.view(1, h, w, 3), tok)
    out_d, marked_d = hip.bg_scene_compose_u8(gctx['image'], fg_d, inner_d, grass_d, sketch_d)
    found = {'sky_color': None, 'sky_bottom': None, 'start_height': None}
    if color_gradient:
        out_d, status_d, info_d = hip.bg_sky_gradient_u8(out_d, inner_d, SEARCH_FROM, SEARCH_HEIGHT)
        hip.bg_scene_overlay_u8(out_d, inner_d, grass_d, sketch_d)
        status, facts = int(status_d.cpu()[0]), info_d.cpu().numpy()       # read together with the image
        if status != 0:
            raise ValueError('scene %s: colour gradient status %d: %s' % (scene.get('image_id', '?'), status,
                                                                          STATUS_TEXT.get(status, 'unknown')))
        c = int(facts[0])
        found = {'sky_color': [c & 255, (c >> 8) & 255, (c >> 16) & 255], 'sky_bottom': int(facts[1]),
                 'start_height': int(facts[2])}
    if info is not None:
        info.update(found)
    if on_device:
        return out_d, marked_d, processed
    return out_d.cpu().numpy(), marked_d.cpu().numpy(), processed
