"""Pick the instances of a user scene that an instruction speaks of (Pipeline_utils/fg_matching_utils.py::
build_instance_matching): the RMI matcher's forward pass and the choice by mask occupancy, on the device
(sketchyscenecolorization_amd/matching.py).

    python match_main.py --snapshot outputs/match_snapshot --image_id 77742204 --instruction 'the bus on the left is yellow'

prints one line ``matched_inst_indices 7,8`` -- what ``obj_colorization_main.py --mode scene ... --inst_indices`` takes -- and
writes <results_dir>/<id>/match.json and <id>_match.png (the prediction on the strokes, x 255).

    python match_main.py --mode eval --snapshot outputs/match_snapshot --dataset val --data_base_dir ../data \
        --captions_base_dir data --seg_data_dir outputs/inst_segm_output_data

scores the checkpoint on a split as Instance_Matching/matching_main.py --mode eval does (sketchyscenecolorization_amd/
match_eval.py): it prints precision@{0.5 .. 0.9}, the overall IoU and mask AP@[0.5:0.95], appends that
block to <eval_result_root>/deeplab_RMI_<split>_result.txt and writes <eval_result_root>/eval_<split>.json.

    python match_main.py --mode train --backbone_snapshot models/SketchyScene_DeepLabv2 --data_base_dir ../data \
        --captions_base_dir data

trains the fusion head on the frozen backbone as Instance_Matching/matching_main.py --mode train does (sketchyscenecolorization_amd/
match_train.py): one (scene, caption) of sentence_instance_train.json per iteration, snapshots
<snapshot_root>/deeplab_RMI_iter_<n>.tfmodel that --mode match and --mode eval read, resumed from when <snapshot_root> holds one.
--scene_cache device keeps every scene's sketch and label map on the device, --scene_cache features the frozen backbone's output
too (sketchyscenecolorization_amd/match_cache.py); --val_freq F scores sentence_instance_val.json every F iterations with the
weights of the moment and appends a line to <log_root>/match_validation.jsonl (match_validation.py).
--val_preview K also writes <log_root>/match_previews/iter_<n>.png and .json at every pass: the first K captions' predictions and
targets over their sketches, made on the device (preview.py); the run is that without it, bit for bit.
--mode eval --visualized 1 writes <visualize_pred_base_dir>/<split>/<id>/<k>_gt.png and <k>_out.png for every caption.

    python match_main.py --mode train --train_backbone 1 --backbone_snapshot models/SketchyScene_DeepLabv2 \
        --data_base_dir ../data --captions_base_dir data

trains the backbone's ResNet/*/DW filters beside the head, through its frozen norms, as RMI_model.py does with
train_fusion_var_only=False (sketchyscenecolorization_amd/match_backbone_train.py).  Its snapshots also
hold the filters' Adam slots; --scene_cache off and device work, features does not (they would be the initial backbone's).

--use_attn 1, in every mode, is the model class's use_attn (RMI_model.py:202-217): a softmax over the word
LSTM's outputs weighs the multimodal LSTM's outputs of every word.  --mode train then also trains attn_fc/DW and attn_fc/biases,
--mode match writes the weights into match.json as "attention"; a snapshot is read with the flag it was trained with.

--weights segnet, in every mode, is the reference's --model segnet (segnet_model.py with is_intermediate):
the SegNet backbone, whose norms take the statistics of the one image, in place of the DeepLab-ResNet.  --mode train then takes
SegNet/* from --backbone_snapshot, trains the head on the frozen backbone (--train_backbone 1 is refused) and writes
segnet_RMI_iter_<n>.tfmodel; --mode eval writes segnet_RMI_<split>_result.txt; a snapshot is read with the --weights it holds."""
import argparse
import json
import os

FLAGS = [
    ('snapshot', str, '', 'directory with a TensorFlow checkpoint file, or a checkpoint prefix'),
    ('vocab_file', str, 'data/match_vocab.txt', "the matcher's word list, one word per line"),
    ('vocab_size', int, 76, 'rows of the embedding'),
    ('text_len', int, 15, 'words the matcher reads'),
    ('scene_dir', str, 'examples', 'directory with sketches/, inner_masks/ and seg_data/'),
    ('scene_size', int, 768, 'side of the scene'),
    ('image_id', str, None, 'the scene'),
    ('instruction', str, '', "e.g. 'the bus on the left is yellow'"),
    ('results_dir', str, 'outputs/match_results', 'where <id>/match.json and <id>/<id>_match.png go'),
    ('use_attn', int, 0, "1: the head with the model class's word attention (use_attn of RMI_model.py), for a checkpoint trained "
                         'with it, and to train one; match.json then holds the weights as "attention"'),
    ('weights', str, 'deeplab', "the backbone, in every mode: 'deeplab' (the DeepLab-ResNet) or 'segnet' (SegNet with the norms of "
                                "the one image); the reference's --model.  'fcn_8s' and 'deeplab_v3plus' are not built"),
]
EVAL_FLAGS = [
    ('data_base_dir', str, '../data', 'eval: the SketchyScene data, with <split>/INSTANCE_GT and <split>/DRAWING_GT'),
    ('captions_base_dir', str, 'data', 'eval: the directory of sentence_instance_<split>.json'),
    ('seg_data_dir', str, 'outputs/inst_segm_output_data', 'eval: the instance segmentation output, <split>/seg_data/<id>_datas.npz'),
    ('max_scenes', int, 0, 'eval: only the first N scenes of the caption file (0: all of them)'),
    ('augment_seed', int, None, 'eval: add random colour attributes to the captions as training does, drawn from random.Random(K); '
                                'default: the captions as they are in the file'),
    ('eval_result_root', str, 'outputs/eval_results', 'eval: where the result block and eval_<split>.json go'),
    ('visualized', int, 0, "eval: 1 to write every caption's target and prediction over the sketch as <k>_gt.png and <k>_out.png "
                           '(plain images: the caption is in captions.json beside them, not drawn as a title)'),
    ('visualize_pred_base_dir', str, 'outputs/visualization', 'eval: where --visualized 1 writes <split>/<image id>/<k>_{gt,out}.png'),
]
TRAIN_FLAGS = [
    ('backbone_snapshot', str, '', 'train: a TensorFlow checkpoint (directory or prefix) with ResNet/*, for a fresh run'),
    ('snapshot_root', str, 'outputs/snapshots', 'train: where the snapshots go; resumed from when it holds a checkpoint file'),
    ('max_iteration', int, 100000, 'train: iterations'),
    ('save_model_freq', int, 10000, 'train: a snapshot every N iterations, and one at the end'),
    ('log_freq', int, 50, 'train: a line every N iterations'),
    ('seed', int, 0, "train: the seed of the tuples' order, of the captions' attributes and of a fresh head"),
    ('start_lr', float, 2.5e-4, 'train: the learning rate at step 0'),
    ('end_lr', float, 1e-5, 'train: the learning rate from --lr_decay_step on'),
    ('lr_decay_step', int, 75000, 'train: steps of the polynomial decay (power 0.9)'),
    ('weight_decay', float, 5e-4, 'train: the rate of the l2 regulariser on every trained DW'),
    ('log_root', str, 'outputs/log', 'train: where match_train.jsonl goes'),
    ('train_fusion_var_only', int, 1, 'train: 1; the backbone is trained with --train_backbone 1'),
    ('train_backbone', int, 0, 'train: 1 to differentiate the backbone as well and update its ResNet/*/DW filters through the frozen '
                               'norms (0: the fusion head alone)'),
    ('training_ignore_bg', int, 1, 'train: 1; the loss over every pixel is not built'),
    ('batch_size', int, 1, 'train: 1'),
    ('gpus', int, 1, 'train: 1'),
    ('graph', int, 0, 'train: 0; the step is not captured'),
    ('keep_prob', float, 1.0, 'train: 1; dropout is not built'),
    ('fusion_type', str, 'RMI', "train: 'RMI'; 'RecurAttn' is not built (the attention that is built is --use_attn 1)"),
    ('summary', int, 0, 'train: 0; event summaries are not written'),
    ('scene_cache', str, 'off', "train: 'off' (every iteration reads its scene's files), 'device' (every scene's sketch and label "
                                "map on the device, read once) or 'features' (and the frozen backbone's output of every scene)"),
    ('val_freq', int, 0, 'train: score sentence_instance_val.json every N iterations and after the last one (0: never)'),
    ('val_scenes', int, 0, 'train: only the first N scenes of sentence_instance_val.json are scored (0: all of them)'),
    ('val_preview', int, 0, 'train: every held-out pass also writes <log_root>/match_previews/iter_<n>.png and .json, the first K '
                            'captions of the pass as overlays on their sketches (0: none; at most 32; needs --val_freq)'),
]
SCENE_CACHE_MODES = ('off', 'device', 'features')


def checked_model(args):
    """The flags that every mode reads -- --use_attn, --weights, --text_len, --scene_size, --vocab_size and --vocab_file: ->
    (config, vocab).  ValueError for a bad one."""
    from sketchyscenecolorization_amd import match_backbones, matching
    if args.use_attn not in (0, 1):
        raise ValueError('--use_attn %d: 0 (the last state feeds the projection) or 1 (the attention-weighted sum of every '
                         "word's state)" % args.use_attn)
    if args.weights not in match_backbones.BACKBONES:
        raise ValueError('--weights %r: only %s (the other backbones are not built)'
                         % (args.weights, ' or '.join(repr(b) for b in match_backbones.BACKBONES)))
    if args.text_len < 1:
        raise ValueError('--text_len %d: at least one word' % args.text_len)
    config = matching.MatchConfig(size=args.scene_size, vocab_size=args.vocab_size, max_len=args.text_len,
                                  use_attn=bool(args.use_attn), backbone=args.weights)
    if not os.path.isfile(args.vocab_file):
        raise ValueError('--vocab_file %r: no such file' % args.vocab_file)
    vocab = matching.load_vocab(args.vocab_file)
    if len(vocab) != args.vocab_size or matching.UNK not in vocab or matching.PAD not in vocab:
        raise ValueError('--vocab_file %r holds %d words, --vocab_size is %d; <unk> and <pad> must be among them'
                         % (args.vocab_file, len(vocab), args.vocab_size))
    return config, vocab


def checked_snapshot_variables(path, config):
    """A snapshot (matching.resolve_snapshot) -> its prefix.  Its variable names are held against the configuration's backbone
    (--weights) and --use_attn, read from its index alone: MatchModel.load_dict's refusals, before anything is allocated."""
    from sketchyscenecolorization_amd import matching, tf_checkpoint
    prefix = matching.resolve_snapshot(path)
    names = {name for name, _shape, _dtype in tf_checkpoint.list_variables(prefix)}
    config.net.check_variables(names)
    matching.check_attention_variables(names, config.use_attn)
    return prefix


def checked_scenes(scenes, data_base_dir, split, more_paths=lambda image_id: (), no_category=None):
    """A split's scenes (match_eval.read_captions): ValueError for a scene without one of its ground-truth files or of
    ``more_paths(image_id)``, for a caption without a word and -- no_category: that message, with %r for the caption -- for one
    that names no category."""
    from sketchyscenecolorization_amd import match_eval, matching
    for image_id, pairs in scenes:
        for path in match_eval.ground_truth_paths(data_base_dir, split, image_id) + tuple(more_paths(image_id)):
            if not os.path.isfile(path):
                raise ValueError('scene %s: %s: no such file' % (image_id, path))
        for caption, _idx in pairs:
            if not matching.sentence_tokens(caption):
                raise ValueError('scene %s: the caption %r holds no word' % (image_id, caption))
            if no_category is not None and match_eval.caption_category(caption)[0] is None:
                raise ValueError('scene %s: %s' % (image_id, no_category % (caption,)))


def reserved_model(cfg):
    """The MatchModel of a configuration.  What its backbone reserves as scratch memory at its first pass is added up first,
    refused as a ValueError when it is more than half of what is free on the device, and printed when there is any."""
    from sketchyscenecolorization_amd import matching
    if cfg.net.scratch_bytes():
        import torch
        print('%s backbone: %d bytes of scratch memory on the device' % (cfg.backbone, cfg.net.check_scratch(torch.cuda.mem_get_info()[0])))
    return matching.MatchModel(cfg)


def agreed_config(config, cfg):
    """A ``config`` handed to ``main`` must be what the flags say: -> config.  ValueError otherwise."""
    if (config.size, config.vocab_size, config.max_len) != (cfg.size, cfg.vocab_size, cfg.max_len):
        raise ValueError('the given configuration and --scene_size / --vocab_size / --text_len disagree')
    if bool(getattr(config, 'use_attn', False)) != cfg.use_attn:
        raise ValueError('the given configuration has use_attn %r, --use_attn is %d' % (config.use_attn, int(cfg.use_attn)))
    if getattr(config, 'backbone', 'deeplab') != cfg.backbone:
        raise ValueError('the given configuration has the backbone %r, --weights is %r' % (config.backbone, cfg.backbone))
    return config


def build_parser():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    for name, typ, default, text in FLAGS + EVAL_FLAGS + TRAIN_FLAGS:
        p.add_argument('--' + name, type=typ, default=default, help=text)
    p.add_argument('--mode', type=str, default='match', help="'match' (one scene and one instruction), 'eval' (a split) or 'train'")
    p.add_argument('--dataset', type=str, default='val', help="eval: the split, 'val' or 'test'")
    p.add_argument('--mask_ap', type=int, default=1, help='eval: 1 to compute mask AP, 0 for IoU and precision only')
    return p


def checked_arguments(args):
    """Every bad argument is a ValueError here, before anything is loaded or written.  -> (config, snapshot prefix, vocab)."""
    from sketchyscenecolorization_amd import matching
    if args.snapshot == '':
        raise ValueError('--snapshot <directory or checkpoint prefix> is needed: the matcher has no weights of its own')
    if args.image_id is None or args.image_id == '' or args.instruction == '':
        raise ValueError("--image_id <id> and --instruction '<text>' are needed")
    if not matching.sentence_tokens(args.instruction):
        raise ValueError('--instruction %r holds no word' % args.instruction)
    config, vocab = checked_model(args)
    prefix = checked_snapshot_variables(args.snapshot, config)
    for sub, name in (('sketches', args.image_id + '.png'), ('inner_masks', args.image_id + '.mat'),
                      ('seg_data', args.image_id + '_datas.npz')):
        if not os.path.isfile(os.path.join(args.scene_dir, sub, name)):
            raise ValueError('--scene_dir %r has no %s/%s' % (args.scene_dir, sub, name))
    return config, prefix, vocab


def checked_eval_arguments(args):
    """--mode eval: every bad argument and every missing file is a ValueError here, before the weights are read or anything is
    written.  -> (config, snapshot prefix, vocab, the scenes of the caption file that will be scored)."""
    from sketchyscenecolorization_amd import match_eval, matching
    if args.snapshot == '':
        raise ValueError('--snapshot <directory or checkpoint prefix> is needed: the matcher has no weights of its own')
    if args.dataset not in ('val', 'test'):
        raise ValueError("--dataset %r: 'val' or 'test'" % args.dataset)
    if args.mask_ap not in (0, 1):
        raise ValueError('--mask_ap %d: 0 or 1' % args.mask_ap)
    if args.max_scenes < 0:
        raise ValueError('--max_scenes %d: a count, 0 for every scene' % args.max_scenes)
    if args.eval_result_root == '':
        raise ValueError('--eval_result_root is empty')
    if args.visualized and args.visualize_pred_base_dir == '':
        raise ValueError('--visualize_pred_base_dir is empty')
    config, vocab = checked_model(args)
    prefix = checked_snapshot_variables(args.snapshot, config)
    scenes = match_eval.read_captions(args.captions_base_dir, args.dataset)
    if args.max_scenes:
        scenes = scenes[:args.max_scenes]
    if not scenes:
        raise ValueError('--captions_base_dir %r: no scene in the caption file of %r' % (args.captions_base_dir, args.dataset))
    checked_scenes(scenes, args.data_base_dir, args.dataset,
                   more_paths=lambda image_id: (match_eval.seg_data_path(args.seg_data_dir, args.dataset, image_id),),
                   no_category=None if args.augment_seed is None else '--augment_seed: the caption %r names no category')
    return config, prefix, vocab, scenes


def evaluate(args, config=None, predicts_out=None):
    """--mode eval.  ``predicts_out``: a path that receives every caption's predicts, uint8 [captions, S, S], as .npy."""
    cfg, prefix, vocab, scenes = checked_eval_arguments(args)
    if config is not None:
        cfg = agreed_config(config, cfg)
    import random
    import numpy as np
    from sketchyscenecolorization_amd import match_eval
    model = reserved_model(cfg)
    model.load_tf_checkpoint(prefix)
    rng = None if args.augment_seed is None else random.Random(args.augment_seed)
    kept = [] if predicts_out is not None else None
    visualizer = None
    if args.visualized:
        from sketchyscenecolorization_amd import preview
        visualizer = preview.EvalVisualizer(args.visualize_pred_base_dir, args.dataset, cfg.size, model.device)
    totals, records = match_eval.evaluate(model, vocab, scenes, args.data_base_dir, args.dataset, args.seg_data_dir,
                                          mask_ap=bool(args.mask_ap), rng=rng, keep_predicts=kept, log=print, visualizer=visualizer)
    model.close()
    block = totals.block(prefix)
    print(block)
    os.makedirs(args.eval_result_root, exist_ok=True)
    with open(os.path.join(args.eval_result_root, '%s_%s_result.txt' % (cfg.net.model_name, args.dataset)), 'a') as f:
        f.write(block)
    record = dict(totals.record(), split=args.dataset, snapshot=prefix, scenes=len(scenes), augment_seed=args.augment_seed,
                  per_caption=records)
    with open(os.path.join(args.eval_result_root, 'eval_%s.json' % args.dataset), 'w') as f:
        json.dump(record, f, indent=1)
    if predicts_out is not None:
        np.save(predicts_out, np.stack(kept))
    return totals


def validation_scenes(args):
    """--val_freq F > 0: the scenes of sentence_instance_val.json that a pass scores; a missing caption file or ground-truth file
    is a ValueError.  None with F = 0: the files of the val split are not looked at.  --seg_data_dir is not read."""
    if args.val_freq == 0:
        return None
    from sketchyscenecolorization_amd import match_validation
    return match_validation.validation_scenes(args.captions_base_dir, args.data_base_dir, args.val_scenes)


def checked_train_arguments(args):
    """--mode train: every bad argument and every missing file of the whole caption file is a ValueError here, before any weight
    is read or anything is written.  -> (config, vocab, training tuples, the snapshot to resume from or None, the backbone's
    checkpoint prefix or None)."""
    from sketchyscenecolorization_amd import match_eval, match_train, matching, preview, tf_checkpoint
    for name, want, why in (('train_fusion_var_only', 1, 'the backbone is trained with --train_backbone 1'),
                            ('training_ignore_bg', 1, 'the loss over every pixel is not built'),
                            ('batch_size', 1, 'the reference trains one tuple per iteration'), ('gpus', 1, 'one device'),
                            ('graph', 0, 'the step is not captured'), ('keep_prob', 1.0, 'dropout is not built'),
                            ('fusion_type', 'RMI', "'RecurAttn' is not built; the attention that is built is --use_attn 1"), ('summary', 0, 'event summaries are not written')):
        if getattr(args, name) != want:
            raise ValueError('--%s %r: only %r (%s)' % (name, getattr(args, name), want, why))
    if args.max_iteration < 1 or args.save_model_freq < 1 or args.log_freq < 1:
        raise ValueError('--max_iteration %d, --save_model_freq %d, --log_freq %d: each at least 1'
                         % (args.max_iteration, args.save_model_freq, args.log_freq))
    if not (args.start_lr > 0 and args.end_lr >= 0 and args.lr_decay_step >= 1 and args.weight_decay >= 0):
        raise ValueError('--start_lr %r, --end_lr %r, --lr_decay_step %d, --weight_decay %r' % (args.start_lr, args.end_lr,
                                                                                             args.lr_decay_step, args.weight_decay))
    if args.snapshot_root == '' or args.log_root == '':
        raise ValueError('--snapshot_root or --log_root is empty')
    if args.scene_cache not in SCENE_CACHE_MODES:
        raise ValueError("--scene_cache %r: 'off', 'device' or 'features'" % args.scene_cache)
    if args.train_backbone not in (0, 1):
        raise ValueError('--train_backbone %d: 0 (the fusion head alone) or 1 (and the backbone)' % args.train_backbone)
    config, vocab = checked_model(args)
    if args.train_backbone and not config.net.trainable:
        raise ValueError('--train_backbone 1 --weights %s: the %s backward is not built; its backbone is run frozen '
                         '(--train_backbone 0)' % (config.backbone, config.net.title))
    if args.train_backbone and args.scene_cache == 'features':
        raise ValueError('--train_backbone 1 --scene_cache features: cached features are those of the initial backbone; '
                         'use --scene_cache device')
    if args.val_freq < 0 or args.val_scenes < 0:
        raise ValueError('--val_freq %d, --val_scenes %d: counts, 0 for never and for every scene' % (args.val_freq, args.val_scenes))
    preview.checked_count(args.val_preview, args.val_freq)
    if vocab[matching.PAD] != 0:
        raise ValueError('--vocab_file %r: <pad> is word %d; training needs it as word 0 (the embedding gradient skips row 0)'
                         % (args.vocab_file, vocab[matching.PAD]))
    resume = backbone = None
    if os.path.exists(os.path.join(args.snapshot_root, 'checkpoint')):
        resume = checked_snapshot_variables(args.snapshot_root, config)     # a resume goes on with the head the snapshot was trained with
        match_train.snapshot_iteration(resume)
        if not os.path.isfile(resume + '.train_state.json'):
            raise ValueError('%s.train_state.json: no such file; the snapshot cannot be resumed from' % resume)
    else:
        if args.backbone_snapshot == '':
            raise ValueError('--backbone_snapshot <directory or checkpoint prefix> is needed: a fresh run takes %s* from it'
                             % config.net.scope)
        backbone = matching.resolve_snapshot(args.backbone_snapshot)
        # a checkpoint of the other backbone is refused from its index; one that lacks a variable, when it is loaded
        config.net.check_variables({name for name, _s, _d in tf_checkpoint.list_variables(backbone)})
    scenes = match_eval.read_captions(args.captions_base_dir, 'train')
    if not scenes:
        raise ValueError('--captions_base_dir %r: no scene in the caption file of the train split' % args.captions_base_dir)
    checked_scenes(scenes, args.data_base_dir, 'train', no_category='the caption %r names no category to add an attribute to')
    validation_scenes(args)
    return config, vocab, match_train.training_tuples(scenes), resume, backbone


def build_caches(args, cfg, model, vocab, tuples):
    """--scene_cache and --val_freq: -> (the MatchSceneCache of the train split or None, the MatchValidation or None).  What the
    two will hold is added up first and refused as a ValueError, before anything is allocated, when it is more than half of what
    is free on the device now."""
    val_scenes = validation_scenes(args)
    if args.scene_cache == 'off' and val_scenes is None:
        return None, None
    import torch
    from sketchyscenecolorization_amd import match_cache, match_validation
    train_scenes = [(image_id, None) for image_id, _caption, _idx in tuples]
    n_train = len(match_cache.distinct_scenes(train_scenes)[0]) if args.scene_cache != 'off' else 0
    n_val = len(match_cache.distinct_scenes(val_scenes)[0]) if val_scenes is not None else 0
    scene_b, feat_b = match_cache.cache_bytes(n_train, cfg.size, cfg.feat_channels if args.scene_cache == 'features' else None)
    val_b = match_cache.cache_bytes(n_val, cfg.size)[0]
    free = torch.cuda.mem_get_info(model.device)[0]
    remedy = 'run with --scene_cache off' if n_train else 'score fewer scenes (--val_scenes N) or none (--val_freq 0)'
    match_cache.check_budget(scene_b + val_b, feat_b, free, remedy_scenes=remedy)
    cache = validation = None
    if args.scene_cache != 'off':
        cache = match_cache.MatchSceneCache(train_scenes, args.data_base_dir, 'train', cfg.size, model.device,
                                            features=model if args.scene_cache == 'features' else None)
        print('scene cache: %d scenes, %d bytes of scenes and %d of features on the device, built in %.1f s'
              % (len(cache), cache.scene_bytes, cache.feature_bytes, cache.build_seconds))
    if val_scenes is not None:
        validation = match_validation.MatchValidation(model, vocab, val_scenes, args.data_base_dir,
                                                      beside=cache.nbytes if cache is not None else 0, preview=args.val_preview)
        print('validation cache: %d scenes, %d captions, %d bytes on the device' % (len(validation.cache), validation.captions,
                                                                                 validation.nbytes))
    return cache, validation


def train(args, config=None):
    """--mode train."""
    cfg, vocab, tuples, resume, backbone = checked_train_arguments(args)
    if config is not None:
        cfg = agreed_config(config, cfg)
    import random
    import numpy as np
    from sketchyscenecolorization_amd import match_eval, match_train, matching, tf_checkpoint
    model = reserved_model(cfg)
    cursor = match_train.TupleCursor(len(tuples), random.Random(args.seed))
    start = 0

    def make_trainer():
        """--train_backbone 1: what the backward will keep is added up first, printed, and refused as a ValueError when it is more
        than half of what is free on the device; then it is all allocated, so that the caches are budgeted beside it."""
        if not args.train_backbone:
            return match_train.MatchTrainer(model, args.weight_decay)
        import torch
        from sketchyscenecolorization_amd import match_backbone_train
        act, scratch, slots = match_backbone_train.check_budget(cfg, torch.cuda.mem_get_info(model.device)[0])
        print('backbone training: %d bytes of kept activations, %d of gradient scratch, %d of gradient and Adam slots on the device'
              % (act, scratch, slots))
        t = match_backbone_train.BackboneMatchTrainer(model, args.weight_decay)
        t.reserve()
        return t
    if resume is not None:
        tensors = tf_checkpoint.read_checkpoint(resume)
        model.load_dict(tensors)
        trainer = make_trainer()
        start = match_train.snapshot_iteration(resume)
        trainer.load_slots(tensors, start)
        with open(resume + '.train_state.json') as f:
            cursor.restore(json.load(f))
        print('loaded', resume)
    else:
        have = tf_checkpoint.read_checkpoint(backbone)
        variables = {k: v for k, v in have.items() if k.startswith(cfg.net.scope)}
        variables.update(match_train.init_head(cfg, args.seed))
        model.load_dict(variables)
        trainer = make_trainer()
        print('firstly train, loaded', backbone)
    print('%d tuples of data.' % len(tuples))
    print('start_iter', start)
    os.makedirs(args.log_root, exist_ok=True)
    log_path = os.path.join(args.log_root, 'match_train.jsonl')
    cache, validation = build_caches(args, cfg, model, vocab, tuples)          # None, None with the defaults
    loss_avg, saved = 0.0, None
    for n_iter in range(start, args.max_iteration):
        image_id, caption_thin, inst_indices = tuples[cursor.next()]
        caption = match_eval.augment_caption(caption_thin, cursor.rng)
        if cache is None:
            gt = match_eval.load_ground_truth(args.data_base_dir, 'train', image_id, cfg.size)
            area = np.bincount(gt['labels'].reshape(-1), minlength=256)
        else:       # no file is read: views of the scene's entry, and the areas that were counted when the cache was built
            gt = cache.entry(image_id)
            area = cache.area[cache.index[image_id]]
        lut = match_train.caption_lut(match_eval.caption_labels(image_id, inst_indices, gt['n_inst'], area))
        indices, seq_len = matching.preprocess_sentence(caption, vocab, cfg.max_len)
        lr = match_train.polynomial_decay(trainer.step_count, args.start_lr, args.end_lr, args.lr_decay_step)
        trainer.step(gt, lut, indices, seq_len, lr)
        if n_iter % args.log_freq == 0 and n_iter != 0:
            loss = trainer.last_loss()
            loss_avg = 0.99 * loss_avg + (1 - 0.99) * loss
            print('iter = %d, loss (cur) = %f, loss (avg) = %f, lr = %f' % (n_iter, loss, loss_avg, lr))
            with open(log_path, 'a') as f:
                f.write(json.dumps({'iter': n_iter, 'loss_cur': loss, 'loss_avg': loss_avg, 'lr': lr, 'image_id': image_id,
                                    'caption': caption}) + '\n')
        if validation is not None and ((n_iter + 1) % args.val_freq == 0 or (n_iter + 1) >= args.max_iteration):
            validation.run_and_log(n_iter + 1, args.log_root)
        if (n_iter + 1) % args.save_model_freq == 0 or (n_iter + 1) >= args.max_iteration:
            saved = match_train.write_snapshot(trainer, args.snapshot_root, n_iter + 1, cursor)
            print('model saved to ' + saved)
    model.close()
    return saved


def main(argv=None, config=None, predicts_out=None):
    """``config``: a MatchConfig other than the released model's (the tests' small models); its size, vocabulary size and
    text length must be the flags'.  ``predicts_out``: --mode eval only, see ``evaluate``."""
    args = build_parser().parse_args(argv)
    from sketchyscenecolorization_amd import preview
    if args.mode != 'train':        # (--mode train holds it against --val_freq, among its own checks)
        preview.checked_count(args.val_preview, args.val_freq, args.mode)
    preview.checked_visualized(args.visualized, args.mode)
    if args.mode == 'eval':
        return evaluate(args, config, predicts_out)
    if args.mode == 'train':
        return train(args, config)
    if args.mode != 'match':
        raise ValueError("--mode %r: 'match', 'eval' or 'train'" % args.mode)
    cfg, prefix, vocab = checked_arguments(args)
    if config is not None:
        cfg = agreed_config(config, cfg)
    import numpy as np
    from PIL import Image
    from sketchyscenecolorization_amd import fg_scene, matching
    scene = fg_scene.load_instances(args.scene_dir, args.image_id, cfg.size)
    matching.pack_masks(scene['boxes'], scene['masks'], cfg.size)       # a bad box is refused before the weights are read
    model = reserved_model(cfg)
    model.load_tf_checkpoint(prefix)
    matched, scores, info = matching.match_instances(model, scene, args.instruction, vocab)
    model.close()
    out_dir = os.path.join(args.results_dir, str(args.image_id))
    os.makedirs(out_dir, exist_ok=True)
    record = {'image_id': str(args.image_id), 'instruction': args.instruction, 'tokens': info['tokens'], 'seq_len': info['seq_len'],
              'matched_inst_indices': matched,
              'occupancy': [None if s != s else float(s) for s in scores.tolist()],
              'class_ids': [int(c) for c in np.asarray(scene['class_ids']).reshape(-1)], 'snapshot': prefix}
    if cfg.use_attn:        # the weights of all --text_len positions, the padded ones included
        record['attention'] = [float(a) for a in info['attention']]
    with open(os.path.join(out_dir, 'match.json'), 'w') as f:
        json.dump(record, f, indent=1)
    Image.fromarray((info['predicts'] != 0).astype(np.uint8) * 255).save(os.path.join(out_dir, '%s_match.png' % args.image_id))
    print('matched_inst_indices ' + ','.join(str(k) for k in matched))
    return matched


if __name__ == '__main__':
    main()
