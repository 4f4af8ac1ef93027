"""The evaluation of the instance matcher on a split (Instance_Matching/matching_main.py --mode eval): overall IoU,
precision@{0.5 .. 0.9} and mask AP@[0.5:0.95] of a checkpoint over the captions of sentence_instance_<split>.json.
DESIGN.md section 8.7.

    per scene    sketch, label map (0: background, k + 1: the k-th ground-truth instance), packed predicted masks -> the device;
                 MatchModel.features (preprocess + backbone) once;
                 area = ssc_label_hist_u8(labels) int64 [256], H = ssc_instance_label_hist(labels, masks) int64 [N,256]
    per caption  MatchModel.predict (head + ssc_match_finish) -> predicts uint8 [S,S] on the device;
                 counts = ssc_instance_occupancy(predicts, masks) int64 [N,2], P = ssc_label_hist_u8(labels, predicts) int64 [256];
                 counts and P go to the host, and every metric is arithmetic on area, H, counts and P

No full-size mask is made on the host and none is multiplied: compute_mask_IU's sums and compute_overlaps_masks' products are
bins of those histograms.  The number types are the reference's (float32 overlaps, float64 scores and thresholds, float32 AP).

Not here: training, visualisation, post_processing_mask_with_segmentation."""
import json
import os

import numpy as np

from . import matching

IOU_LEVELS = (.5, .6, .7, .8, .9)                   # eval_seg_iou_list
AP_THRESHOLDS = np.linspace(.5, .95, 10)            # float64, as the reference's compute_ap receives them
MAX_INSTANCES = 255                                 # labels are bytes, 0 is the background

# ---------------------------------------------------------------------------------------------------------------------------
# caption augmentation (text_processing.py::augment_the_caption_with_attr)
# ---------------------------------------------------------------------------------------------------------------------------
COLOR_LIST = ['dark brown', 'light brown', 'light gray', 'dark gray', 'black', 'red', 'dark green', 'light green', 'dark blue',
              'light blue', 'yellow', 'orange', 'pink', 'purple']
CATEGORIES = ['bench', 'bird', 'bus', 'butterfly', 'car', 'cat', 'chair', 'chicken', 'cloud', 'cow', 'dog', 'duck', 'horse', 'house',
              'grass', 'moon', 'person', 'pig', 'rabbit', 'road', 'sheep', 'star', 'sun', 'tree', 'truck']
CATEGORIES_PLURAL = ['benches', 'birds', 'buses', 'butterflies', 'cars', 'cats', 'chairs', 'chickens', 'clouds', 'cows', 'dogs',
                     'ducks', 'horses', 'houses', 'grasses', 'moons', 'people', 'pigs', 'rabbits', 'roads', 'sheep', 'stars', 'suns',
                     'trees', 'trucks']
PLURAL_WORDS = ['both', 'all', 'two', 'three', 'four', 'five', 'six']
CATEGORY_COLORS = {
    'bench': ['light brown', 'dark brown', 'yellow', 'orange', 'dark blue', 'light blue', 'red', 'pink', 'purple'],
    'cat': ['yellow', 'orange', 'dark gray', 'pink', 'light gray'],
    'chair': ['light brown', 'dark brown'],
    'cloud': ['dark gray', 'light blue', 'dark blue'],
    'dog': ['light brown', 'dark brown', 'orange'],
    'duck': ['yellow', 'orange'],
    'grass': ['dark green', 'light green'],
    'horse': ['light brown', 'dark brown', 'orange', 'dark gray', 'light gray', 'dark blue', 'purple'],
    'moon': ['yellow', 'orange'],
    'pig': ['pink', 'red'],
    'rabbit': ['pink', 'dark gray'],
    'road': ['yellow', 'orange', 'dark gray', 'black', 'light brown', 'dark brown'],
    'sheep': ['red', 'yellow', 'dark blue', 'light blue', 'orange', 'pink', 'light green', 'dark green', 'purple', 'cyan', 'dark brown',
              'dark gray', 'light brown', 'light gray', 'black'],
    'star': ['yellow', 'orange', 'red'],
    'sun': ['yellow'],
    'tree': ['light green', 'dark green'],
    'truck': ['red', 'yellow', 'orange', 'light green', 'dark blue', 'light blue'],
    'chicken': ['yellow', 'orange', 'light brown', 'dark brown'],
    'cow': ['light brown', 'dark brown', 'yellow', 'dark gray', 'light gray'],
}


def caption_category(caption):
    """-> (the first category word of the caption in its singular form or None, whether the caption speaks of several): a plural
    word in front of the category ('two', 'all', ..) or the category's plural form makes it several.  The search ends at the
    first category word ('sheep' is found as a singular)."""
    words = [w.lower() for w in matching._SPLIT.split(caption.strip()) if len(w.strip()) > 0 and w != '-']
    several = False
    for w in words:
        if w in PLURAL_WORDS:
            several = True
        if w in CATEGORIES:
            return w, several
        if w in CATEGORIES_PLURAL:
            return CATEGORIES[CATEGORIES_PLURAL.index(w)], True
    return None, several


def augment_caption(caption, rng):
    """'the dog on the left' -> 'the dog on the left is dark brown': the caption with a random colour attribute.  ``rng`` is a
    ``random.Random`` (or the ``random`` module); it is consumed as the reference consumes ``random`` -- two colour draws first,
    always; then the kind for a person (3), a bus / car / house (2) or a bird (2); none for a butterfly; one draw from the
    category's own colours for every other category -- so that a seeded generator gives the reference's captions.  ValueError
    for a caption without a category word."""
    category, several = caption_category(caption)
    if category is None:
        raise ValueError('%r names no category that an attribute could be added to' % (caption,))
    c0 = COLOR_LIST[rng.randint(0, len(COLOR_LIST) - 1)]
    c1 = COLOR_LIST[rng.randint(0, len(COLOR_LIST) - 1)]
    verb = ' are' if several else ' is'
    if category == 'person':
        kind = rng.randint(0, 2)
        if kind == 0:
            return caption + verb + ' in ' + c0
        return caption + verb + ' in ' + c0 + ' shirt and ' + c1 + (' pants' if kind == 1 else ' skirt')
    if category in ('bus', 'car', 'house'):
        if rng.randint(0, 1) == 0:
            return caption + verb + ' ' + c0
        return caption + verb + ' ' + c0 + ' with ' + c1 + (' roof' if category == 'house' else ' windows')
    if category == 'bird':
        if rng.randint(0, 1) == 0:
            return caption + verb + ' ' + c0
        return caption + verb + ' ' + c0 + ' with ' + c1 + ' wings'
    if category == 'butterfly':
        return caption + (' have' if several else ' has') + ' ' + c0 + ' body and ' + c1 + ' wings'
    own = CATEGORY_COLORS[category]
    return caption + verb + ' ' + own[rng.randint(0, len(own) - 1)]


# ---------------------------------------------------------------------------------------------------------------------------
# ground truth and predicted instances (sketch_data_processing.py::load_data_gt, load_mask, get_pred_instance_mask)
# ---------------------------------------------------------------------------------------------------------------------------
def label_map(instance_gt):
    """INSTANCE_GT (integers, 0: background) -> (uint8 label map: 1 + the rank of a pixel's instance id among the ids that own a
    pixel, 0 for the background; the ids in that order).  The rank is the reference's real_instanceIdx, which the caption
    file's inst_indices index.  ValueError for more than 255 instances."""
    gt = np.asarray(instance_gt)
    if gt.ndim != 2 or gt.dtype.kind not in 'iub':
        raise ValueError('INSTANCE_GT is %s %s: a 2-d integer image is needed' % (gt.dtype, gt.shape))
    gt = gt.astype(np.int64)
    if gt.min() < 0:
        raise ValueError('INSTANCE_GT holds the negative id %d' % int(gt.min()))
    ids = np.unique(gt)
    ids = ids[ids != 0]
    if len(ids) > MAX_INSTANCES:
        raise ValueError('%d instances: a label map of bytes holds %d at the most' % (len(ids), MAX_INSTANCES))
    table = np.zeros(int(gt.max()) + 1, dtype=np.uint8)
    table[ids] = np.arange(1, len(ids) + 1, dtype=np.uint8)
    return table[gt], [int(i) for i in ids]


def zoom_labels(labels, size):
    """The label map at size x size by scipy.ndimage.zoom(order=0), the reference's scaling of its masks.  Nearest sampling picks
    one source pixel per output pixel, so this is the zoom of every instance's mask at once."""
    import scipy.ndimage
    labels = np.ascontiguousarray(labels, dtype=np.uint8)
    if labels.shape[0] != labels.shape[1]:
        raise ValueError('the label image is %s: the matcher evaluates square scenes' % (labels.shape,))
    if labels.shape[0] == size:
        return labels
    scale = size / labels.shape[0]
    out = np.ascontiguousarray(scipy.ndimage.zoom(labels, zoom=[scale, scale], order=0), dtype=np.uint8)
    if out.shape != (size, size):
        raise ValueError('the zoom of a %d x %d label image by %r is %s, not %d x %d' % (labels.shape + (scale, out.shape, size, size)))
    return out


def ground_truth_paths(data_base_dir, split, image_id):
    base = os.path.join(data_base_dir, split)
    return (os.path.join(base, 'INSTANCE_GT', 'sample_%s_instance.mat' % image_id),
            os.path.join(base, 'DRAWING_GT', 'L0_sample%s.png' % image_id))


def seg_data_path(seg_data_dir, split, image_id):
    return os.path.join(seg_data_dir, split, 'seg_data', '%s_datas.npz' % image_id)


def load_ground_truth(data_base_dir, split, image_id, size):
    """-> {image_id, sketch uint8 [S,S,3] (RGB, NEAREST to S), labels uint8 [S,S], n_inst}.  CLASS_GT is not read: the evaluation
    never uses the classes of the ground truth."""
    import scipy.io
    from PIL import Image
    mat, png = ground_truth_paths(data_base_dir, split, image_id)
    for p in (mat, png):
        if not os.path.isfile(p):
            raise ValueError('scene %s: %s: no such file' % (image_id, p))
    try:
        labels, ids = label_map(scipy.io.loadmat(mat)['INSTANCE_GT'])
    except ValueError as e:
        raise ValueError('scene %s: %s' % (image_id, e))
    image = Image.open(png).convert('RGB')
    if image.width != size or image.height != size:
        image = image.resize((size, size), resample=Image.NEAREST)
    return {'image_id': str(image_id), 'sketch': np.ascontiguousarray(np.array(image, dtype=np.uint8)),
            'labels': zoom_labels(labels, size), 'n_inst': len(ids)}


def load_pred_instances(seg_data_dir, split, image_id, size):
    """<seg_data_dir>/<split>/seg_data/<id>_datas.npz -> {boxes int32 [N,4], masks, class_ids, buf, offsets}, checked and packed
    by matching.pack_masks (ValueError for a bad box or mask)."""
    path = seg_data_path(seg_data_dir, split, image_id)
    if not os.path.isfile(path):
        raise ValueError('scene %s: %s: no such file' % (image_id, path))
    with np.load(path, allow_pickle=True) as npz:
        for key in ('pred_masks', 'pred_boxes', 'pred_class_ids'):
            if key not in npz.files:
                raise ValueError('scene %s: %s has no %s' % (image_id, path, key))
        boxes = np.array(npz['pred_boxes'], dtype=np.int32).reshape(-1, 4)
        masks = [np.ascontiguousarray(m, dtype=np.uint8) for m in npz['pred_masks']]
        class_ids = np.array(npz['pred_class_ids'], dtype=np.int32).reshape(-1)
    if len(class_ids) != len(boxes):
        raise ValueError('scene %s: %d boxes and %d classes' % (image_id, len(boxes), len(class_ids)))
    try:
        buf, offsets = matching.pack_masks(boxes, masks, size)
    except ValueError as e:
        raise ValueError('scene %s: %s' % (image_id, e))
    return {'boxes': boxes, 'masks': masks, 'class_ids': class_ids, 'buf': buf, 'offsets': offsets}


def read_captions(captions_base_dir, split):
    """sentence_instance_<split>.json -> [(image id, [(caption, inst_indices), ..] in the file's order), ..]."""
    path = os.path.join(captions_base_dir, 'sentence_instance_%s.json' % split)
    if not os.path.isfile(path):
        raise ValueError('%s: no such file' % path)
    with open(path) as f:
        data = json.load(f)
    out = []
    for entry in data:
        if 'key' not in entry or 'sen_instIdx_map' not in entry:
            raise ValueError('%s: an entry without key / sen_instIdx_map' % path)
        pairs = [(str(c), [int(i) for i in idx]) for c, idx in entry['sen_instIdx_map'].items()]
        for c, idx in pairs:
            if not idx:
                raise ValueError('%s: scene %s: the caption %r lists no instance' % (path, entry['key'], c))
        out.append((str(entry['key']), pairs))
    return out


def caption_labels(image_id, inst_indices, n_inst, area):
    """The labels of a caption's instances, as listed (duplicates stay).  ValueError naming the scene for an index outside the
    scene's instances and for an instance that the zoom left without a pixel."""
    labels = []
    for i in inst_indices:
        if not 0 <= int(i) < n_inst:
            raise ValueError('scene %s: instance index %d, the scene has %d instances' % (image_id, int(i), n_inst))
        if int(area[int(i) + 1]) == 0:
            raise ValueError('scene %s: instance %d has no pixel left after the zoom' % (image_id, int(i)))
        labels.append(int(i) + 1)
    return labels


# ---------------------------------------------------------------------------------------------------------------------------
# the metrics, on integer histograms (eval_tools.py)
# ---------------------------------------------------------------------------------------------------------------------------
def mask_iu(P, area, labels):
    """compute_mask_IU(predicts, target) with target the union of the caption's instances: I = sum of P over the target's labels,
    U = every predicted pixel + the target's area - I.  Python integers."""
    P, area = np.asarray(P, dtype=np.int64), np.asarray(area, dtype=np.int64)
    target = sorted(set(int(g) for g in labels))
    inter = int(P[target].sum())
    return inter, int(P.sum()) + int(area[target].sum()) - inter


def overlaps_f32(H, area, labels):
    """compute_overlaps_masks(pred_masks, gt_masks) float32 [len(H), len(labels)]: the intersection of predicted instance k with
    the instance of label g is H[k][g], the areas are sum_g H[k][g] and area[g].  float32 sums, difference and quotient as in the
    reference; counts below 2^24 are exact in float32."""
    H = np.asarray(H, dtype=np.int64).reshape(-1, 256)
    labels = [int(g) for g in labels]
    inter = H[:, labels].astype(np.float32)
    area1 = H.sum(axis=1).astype(np.float32)
    area2 = np.asarray(area, dtype=np.int64)[labels].astype(np.float32)
    union = area1[:, None] + area2[None, :] - inter
    with np.errstate(divide='ignore', invalid='ignore'):
        return inter / union


def descending(values):
    """The order of a reversed stable ascending sort: descending, and of equal values the later one first."""
    return np.argsort(values, kind='stable')[::-1]


def average_precision(scores, overlaps, threshold):
    """compute_ap: scores float64 [n], overlaps float32 [n, nGT] in the same order, the threshold a float64.  The predictions in
    ``descending`` order of score each take the unmatched ground-truth instance they overlap most (``descending`` again) if that
    overlap, widened from float32, is not below the threshold; then the precision envelope over the recall steps."""
    overlaps = np.asarray(overlaps, dtype=np.float32)
    n, n_gt = overlaps.shape
    overlaps = overlaps[descending(np.asarray(scores, dtype=np.float64))]
    pred_match, gt_match = np.zeros(n), np.zeros(n_gt)
    for i in range(n):
        for j in descending(overlaps[i]):
            if gt_match[j] == 1:
                continue
            if np.float64(overlaps[i, j]) < np.float64(threshold):
                break
            gt_match[j] = pred_match[i] = 1
            break
    hits = np.cumsum(pred_match)
    precisions = np.concatenate([[0.], hits / (np.arange(n) + 1), [0.]])
    recalls = np.concatenate([[0.], (hits.astype(np.float32) / np.float32(n_gt)).astype(np.float64), [1.]])    # float32 recalls
    for i in range(len(precisions) - 2, -1, -1):
        precisions[i] = max(precisions[i], precisions[i + 1])
    steps = np.where(recalls[:-1] != recalls[1:])[0] + 1
    return float(np.sum((recalls[steps] - recalls[steps - 1]) * precisions[steps]))


def caption_ap(counts, H, area, labels):
    """-> (matched instance indices, their float64 scores, float32 [10] = the AP at every threshold of AP_THRESHOLDS; zeros when
    nothing was predicted).  The predictions are matching.select_instances': occupancy above 0.5, the occupancy as the score."""
    matched, scores = matching.select_instances(counts)
    ap = np.zeros(len(AP_THRESHOLDS), dtype=np.float32)
    if matched:
        ov = overlaps_f32(np.asarray(H, dtype=np.int64).reshape(-1, 256)[matched], area, labels)
        for j, t in enumerate(AP_THRESHOLDS):
            ap[j] = average_precision(scores[matched], ov, t)
    return matched, scores[matched], ap


class Totals(object):
    """What the evaluation adds up over the captions."""

    def __init__(self, mask_ap=True):
        self.mask_ap = bool(mask_ap)
        self.cum_I = self.cum_U = self.captions = 0
        self.correct = [0] * len(IOU_LEVELS)
        self.aps = []

    def add(self, I, U, ap=None):
        self.cum_I += int(I)
        self.cum_U += int(U)
        self.captions += 1
        for k, t in enumerate(IOU_LEVELS):
            self.correct[k] += int(I / U >= t)         # float64, as the reference
        if self.mask_ap:
            self.aps.append(np.asarray(ap, dtype=np.float32))

    def overall_iou(self):
        return self.cum_I / self.cum_U

    def precision(self):
        return [c / float(self.captions) for c in self.correct]

    def mean_ap(self):
        """(mAP, mAP_list [10]): float64 means of the float32 AP vectors (the reference takes these means in float32)."""
        a = np.asarray(self.aps, dtype=np.float64).reshape(-1, len(AP_THRESHOLDS))
        return float(a.mean()), a.mean(axis=0)

    def block(self, snapshot):
        """The reference's result block."""
        s = '\n' + snapshot + '\nSegmentation evaluation (without DenseCRF):\n'
        for t, p in zip(IOU_LEVELS, self.precision()):
            s += 'precision@%s = %f\n' % (str(t), p)
        s += 'overall IoU = %f\n' % self.overall_iou()
        if self.mask_ap:
            m, ml = self.mean_ap()
            s += 'iou_threshold %s,  mAP = %s\n' % ('@[0.5:0.95]', str(np.float64(m)))
            s += 'mAP_list = %s\n' % str(ml)
        return s

    def record(self):
        r = {'captions': self.captions, 'cum_I': self.cum_I, 'cum_U': self.cum_U, 'overall_IoU': self.overall_iou(),
             'precision': {str(t): p for t, p in zip(IOU_LEVELS, self.precision())}}
        if self.mask_ap:
            m, ml = self.mean_ap()
            r.update(mAP=m, mAP_list=[float(v) for v in ml])
        return r


# ---------------------------------------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------------------------------------
class SceneOnDevice(object):
    """A scene's label map and packed predicted masks on the device, and what does not depend on the caption: area int64 [256]
    and H int64 [N,256], on the host."""

    def __init__(self, image_id, labels, boxes, buf, offsets, n_inst, device='cuda'):
        import torch
        from . import hip
        labels = np.ascontiguousarray(labels, dtype=np.uint8)
        if labels.ndim != 2 or labels.shape[0] != labels.shape[1]:
            raise ValueError('scene %s: the label map is %s' % (image_id, labels.shape))
        if int(labels.max()) > int(n_inst):
            raise ValueError('scene %s: label %d in a scene of %d instances' % (image_id, int(labels.max()), int(n_inst)))
        self.image_id, self.n_inst, self.size = str(image_id), int(n_inst), int(labels.shape[0])
        self.labels = torch.from_numpy(labels).to(device)
        self.buf = torch.from_numpy(np.ascontiguousarray(buf, dtype=np.uint8)).to(device)
        self.boxes = torch.from_numpy(np.ascontiguousarray(boxes, dtype=np.int32).reshape(-1, 4)).to(device)
        self.offsets = torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.int64)).to(device)
        self.n_pred = int(self.boxes.shape[0])
        area = hip.label_hist_u8(self.labels)
        H = hip.instance_label_hist(self.labels, self.buf, self.boxes, self.offsets)
        self.counts = torch.empty((self.n_pred, 2), dtype=torch.int64, device=device)
        self.P = torch.empty(256, dtype=torch.int64, device=device)
        self.area, self.H = area.cpu().numpy(), H.cpu().numpy()
        if (self.H < 0).any():
            raise RuntimeError('ssc_instance_label_hist refused instance %d' % int(np.nonzero(self.H[:, 0] < 0)[0][0]))


def upload_scene(gt, pred, device='cuda'):
    """load_ground_truth's and load_pred_instances' dicts -> SceneOnDevice."""
    return SceneOnDevice(gt['image_id'], gt['labels'], pred['boxes'], pred['buf'], pred['offsets'], gt['n_inst'], device)


def score_caption(predicts_d, scene, inst_indices, mask_ap=True):
    """predicts uint8 [S,S] on the device (anyone's: the matcher's, or a test's), a SceneOnDevice, the caption's inst_indices ->
    {I, U, matched, scores, ap}: ssc_instance_occupancy and ssc_label_hist_u8 gated by predicts on the device, their integers
    copied to the host, the metrics from those."""
    from . import hip
    if tuple(predicts_d.shape) != (scene.size, scene.size):
        raise ValueError('predicts is %s, the scene %d x %d' % (tuple(predicts_d.shape), scene.size, scene.size))
    labels = caption_labels(scene.image_id, inst_indices, scene.n_inst, scene.area)
    hip.label_hist_u8(scene.labels, predicts_d, out=scene.P)
    if mask_ap:
        hip.instance_occupancy(predicts_d, scene.buf, scene.boxes, scene.offsets, out=scene.counts)
    P = scene.P.cpu().numpy()
    I, U = mask_iu(P, scene.area, labels)
    out = {'I': I, 'U': U, 'P': P}
    if mask_ap:
        counts = scene.counts.cpu().numpy()
        if (counts < 0).any():
            raise RuntimeError('ssc_instance_occupancy refused instance %d' % int(np.nonzero(counts[:, 0] < 0)[0][0]))
        matched, scores, ap = caption_ap(counts, scene.H, scene.area, labels)
        out.update(counts=counts, matched=matched, scores=scores, ap=ap)
    return out


def evaluate(model, vocab, scenes, data_base_dir, split, seg_data_dir, mask_ap=True, rng=None, keep_predicts=None, log=None,
             visualizer=None):
    """scenes: read_captions' list (cut to what is wanted).  The backbone runs once per scene, the head once per caption.
    ``rng``: a random.Random for augment_caption, None for the captions as they are.  ``keep_predicts``: a list that receives
    every caption's predicts (host, uint8).  ``visualizer``: a preview.EvalVisualizer that writes every caption's target and
    prediction over the sketch (--visualized 1); it reads predicts and the label map and changes no number.
    -> (Totals, per-caption records)."""
    size, T = model.cfg.size, model.cfg.max_len
    totals, records = Totals(mask_ap), []
    for n, (image_id, pairs) in enumerate(scenes):
        if log is not None:
            log('Processing %d / %d , img_idx: %s' % (n + 1, len(scenes), image_id))
        gt = load_ground_truth(data_base_dir, split, image_id, size)
        pred = load_pred_instances(seg_data_dir, split, image_id, size)
        scene = upload_scene(gt, pred, model.device)
        for _caption, idx in pairs:
            caption_labels(image_id, idx, scene.n_inst, scene.area)         # a bad caption is refused before the backbone runs
        feat, stroke = model.features(gt['sketch'])
        if visualizer is not None:
            visualizer.scene(image_id, gt['sketch'])
        for k, (caption, inst_indices) in enumerate(pairs):
            text = caption if rng is None else augment_caption(caption, rng)
            indices, seq_len = matching.preprocess_sentence(text, vocab, T)
            _up, predicts = model.predict(feat, stroke, indices, seq_len)
            got = score_caption(predicts, scene, inst_indices, mask_ap)
            totals.add(got['I'], got['U'], got.get('ap'))
            rec = {'image_id': image_id, 'caption': caption, 'text': text, 'inst_indices': list(inst_indices), 'I': got['I'],
                   'U': got['U']}
            if mask_ap:
                rec.update(matched_inst_indices=got['matched'], AP=[float(v) for v in got['ap']])
            records.append(rec)
            if keep_predicts is not None:
                keep_predicts.append(predicts.cpu().numpy())
            if visualizer is not None:
                from . import match_train
                visualizer.caption(k, caption, text, predicts, scene.labels,
                                   match_train.caption_lut(caption_labels(image_id, inst_indices, scene.n_inst, scene.area)))
    if visualizer is not None:
        visualizer.finish()
    return totals, records
