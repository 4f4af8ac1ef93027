#!/usr/bin/env python
"""Command line of the Foreground_Instance_Colorization module on the MI355X-native HIP path.

Drop-in for the reference CLI (obj_colorization_main.py:159-257): the same flags, short aliases, defaults and
choices, the same run directory ``outputs/<UTC Y-m-d-H-M-S>/{log,snapshot,validation_results,test_results,
inference_results}``, ``log/param_<first iteration>.json`` and the restart-after-NaN loop.

    python obj_colorization_main.py --mode train --block_type Pix2Pix --batch_size 32 --max_iter 1000
    python obj_colorization_main.py --mode train -bt Pix2Pix -gpu 8      # starts itself as 8 ranks, one per GPU
    python obj_colorization_main.py --mode train -bt Pix2Pix -bs 32 -rc device   # data/tfrecord/train cached on the GPU
    python -m torch.distributed.run --nproc-per-node 8 obj_colorization_main.py --mode train -bt Pix2Pix -gpu 8   # same
    python obj_colorization_main.py --mode val -rf <timestamp> -bt Pix2Pix -mt 1   # validation PNGs and their metrics.json
    python obj_colorization_main.py --mode train -bt Pix2Pix -bs 32 -rc device -vf 1000   # data/tfrecord/val scored every 1000
    python obj_colorization_main.py --mode inference -rf <timestamp> --infer_name car.png \
        --instruction 'the car is yellow with blue window'
    python obj_colorization_main.py --mode scene -rf <timestamp> --image_id 77742204 --inst_indices 7,8 \
        --instruction 'the bus on the left is yellow with blue windows'

--mode scene paints the named instances of one user scene as the reference's scene pipeline does (Pipeline_utils/fg_color_utils.py
::build_instance_colorization): ``<scene_dir>/sketches/<id>.png``, ``inner_masks/<id>.mat`` and ``seg_data/<id>_datas.npz`` are
read, the instruction is cut down to 'the <category> is ...', every instance goes through a forward pass of its own and is pasted
into --previous_image (default: the sketch) on the device (sketchyscenecolorization_amd/fg_scene.py).
``outputs/<timestamp>/scene_results/<id>/`` receives ``<id>_inst.png`` and ``scene.json``; nothing is written when the call fails.
The reference's Instance_Matching step is not part of this: the caller names the instances.  bg_colorization_main.py --mode scene
takes the result as its --previous_image, and the other way round.
"""
import argparse
import json
import os

os.environ.setdefault('HIP_FORCE_DEV_KERNARG', '1')     # kernel arguments in device memory (measured: 1570 vs 1540 images/s with 0)
import time

from sketchyscenecolorization_amd.obj_lib import main_procedure
from sketchyscenecolorization_amd.obj_lib.config import Config

# (long flag, short flag, type, default, choices, Config / d_params key, help)
FLAGS = [
    ('mode', 'md', str, 'train', ['train', 'val', 'test', 'inference', 'scene'], 'dataset_type', 'what to run'),
    ('resume_from', 'rf', str, '', None, 'resume_from', 'timestamp of an earlier run under outputs/ to continue or evaluate'),
    ('batch_size', 'bs', int, 2, None, 'batch_size', 'samples per GPU and step'),
    ('max_iter', 'mi', int, 100000, None, 'max_iter_step', 'last training iteration'),
    ('optimizer', 'opt', str, 'Adam', ['RMSprop', 'Adam', 'AdaDelta', 'AdaGrad'], 'optimizer', 'optimizer family'),
    ('lr_G', 'lrg', float, 2e-4, None, 'lr_G', 'generator step size'),
    ('lr_D', 'lrd', float, 1e-4, None, 'lr_D', 'discriminator step size'),
    ('small_img', 'si', int, 0, [0, 1], 'small_img', '1 = 64x64 instances instead of 192x192'),
    ('lstm_hybrid', 'lh', int, 1, [0, 1], 'LSTM_hybrid', '1 = the caption steers the colours'),
    ('distance_map', 'dm', int, 0, [0, 1], 'distance_map', '1 = sketches as distance maps'),
    ('block_type', 'bt', str, 'MRU', ['MRU', 'Pix2Pix', 'Residual'], 'block_type', 'network family'),
    ('vocab_size', 'vs', int, 58, None, 'vocab_size', 'caption vocabulary size'),
    ('disc_iterations', 'di', int, 1, None, 'disc_iterations', 'discriminator updates per generator update'),
    ('ld', 'ld', int, 10, None, 'ld', 'gradient-penalty weight (unused by the live loss)'),
    ('num_gpu', 'gpu', int, 1, None, 'num_gpu', 'towers (one process per GPU under torch.distributed.run)'),
    ('extra_info', 'ei', str, '', None, 'extra_info', 'free text stored with the run parameters'),
    ('summary_write_freq', 'swf', int, 100, None, 'summary_write_freq', 'iterations between scalar summaries'),
    ('save_model_freq', 'smf', int, 10000, None, 'save_model_freq', 'iterations between snapshots'),
    ('count_left_time_freq', 'clt', int, 100, None, 'count_left_time_freq', 'iterations between ETA prints'),
    ('count_inception_score_freq', 'cis', int, -1, None, 'count_inception_score_freq', '-1 = never'),
    ('infer_name', 'in', str, '', None, 'infer_name', 'sketch file under examples/ (inference mode)'),
    ('instruction', 'ins', str, '', None, 'instruction', 'caption for that sketch (inference mode)'),
    ('record_cache', 'rc', str, 'off', ['off', 'device'], 'record_cache',
     'device = train from data/tfrecord/train held on the GPU as uint8 (0.88 MB per record, 2.2 MB with --distance_map 1)'),
    ('metrics', 'mt', int, 0, [0, 1], 'metrics',
     '1 (--mode val): score every output against its target on the GPU (MAE, PSNR, SSIM) and write metrics.json beside the PNGs'),
    ('val_freq', 'vf', int, 0, None, 'val_freq',
     'iterations between held-out passes during training: data/tfrecord/val scored on the GPU (MAE, PSNR, SSIM), one line per '
     'pass in log/validation.jsonl; 0 = never'),
    ('val_records', 'vn', int, 0, None, 'val_records', 'held-out records a pass takes, the first N in file order; 0 = all'),
    ('val_preview', 'vp', int, 0, None, 'val_preview',
     'every held-out pass (needs -vf F > 0) also writes log/previews/step_<step>.png and .json: a row for each of the first K '
     'records with its sketch, the output of the pass and its target, made on the GPU; at most 32; 0 = none.  Under '
     '--distance_map 1 the cache keeps no sketch bytes and the sketch column is left out'),
    ('color_metrics', 'cm', int, 0, [0, 1], 'color_metrics',
     '1: colour scores beside MAE / PSNR / SSIM, made on the GPU: CIELAB dE76, its chroma and lightness parts, the intersection '
     'of the ab histograms, colourfulness of output and target.  --mode val (needs -mt 1) writes color_metrics.json beside '
     'metrics.json; --mode train (needs -vf F > 0) adds a "color" key to every line of log/validation.jsonl'),
]
# --mode scene only: (long flag, short flag, type, default, help); not part of the run parameters
SCENE_FLAGS = [
    ('scene_dir', 'sd', str, 'examples', 'directory with sketches/, inner_masks/ and seg_data/'),
    ('scene_size', 'ss', int, 768, 'square size of the scene (the inner mask has it, the sketch is brought to it)'),
    ('image_id', 'id', str, None, 'the scene, <id> of sketches/<id>.png'),
    ('inst_indices', 'ii', str, None, "the instances to paint, comma-separated indices into the scene's segmentation data"),
    ('previous_image', 'pi', str, '', 'the result of the last instruction, a png of the scene size (default: the sketch)'),
    ('noise_seed', 'ns', int, -1, '-1: noise drawn on the device as inference mode draws it; n >= 0: the p-th instance of the '
                                  'call gets torch.randn(1, 256, generator=torch.Generator().manual_seed(n + p))'),
]
RESULT_DIRS = {'val': 'validation_results', 'test': 'test_results', 'inference': 'inference_results', 'scene': 'scene_results'}


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    for name, short, typ, default, choices, _key, text in FLAGS:
        parser.add_argument('--' + name, '-' + short, type=typ, default=default, choices=choices, help=text)
    for name, short, typ, default, text in SCENE_FLAGS:
        parser.add_argument('--' + name, '-' + short, type=typ, default=default, help='--mode scene: ' + text)
    return parser


def run_dirs(stamp):
    root = os.path.join('outputs', stamp)
    return os.path.join(root, 'log'), os.path.join(root, 'snapshot'), root


def is_stamp(text):
    return bool(text) and len(text.split('-')) == 6


def start_or_resume_training(params):
    """One call of main_procedure.train: fresh run (new UTC stamp) or continuation of ``resume_from``."""
    stamp = params['resume_from']
    fresh = stamp is None or stamp == ''
    rank, multi = int(os.environ.get('RANK', 0)), params['num_gpu'] > 1
    if multi:       # one process per GPU: rank 0 decides the run directory and the first iteration for everyone
        from sketchyscenecolorization_amd.dist_utils import init_distributed
        dist = init_distributed()
    if fresh:
        stamp = time.strftime('%Y-%m-%d-%H-%M-%S', time.gmtime())
        first_iter = 0
    elif not is_stamp(stamp):
        print('Invalid resume folder')
        return None, stamp
    if multi and fresh:     # ranks that straddle a second boundary would otherwise write to different directories
        box = [stamp]
        dist.broadcast_object_list(box, src=0)
        stamp = box[0]
    log_dir, ckpt_dir, _ = run_dirs(stamp)
    if fresh:
        for d in (log_dir, ckpt_dir):
            os.makedirs(d, exist_ok=True)
    else:
        box = [None]
        if rank == 0:
            latest = main_procedure.latest_checkpoint(ckpt_dir)
            box = [None if latest is None else int(os.path.basename(latest).split('-')[1]) + 1]
        if multi:
            dist.broadcast_object_list(box, src=0)
        if box[0] is None:
            raise RuntimeError('no snapshot under %s' % ckpt_dir)
        first_iter = box[0]
    params.update(log_dir=log_dir, ckpt_dir=ckpt_dir, iter_from=first_iter)
    if int(os.environ.get('RANK', 0)) == 0:
        os.makedirs(log_dir, exist_ok=True)     # a released model dropped into outputs/<stamp>/snapshot has no log/ yet
        with open(os.path.join(log_dir, 'param_%d.json' % first_iter), 'w') as fp:
            json.dump(params, fp, indent=4)
    Config.set_from_dict(params)
    print(('Launching new train: %s' if fresh else 'Launching training from checkpoint: %s') % stamp)
    return main_procedure.train(**params), stamp


def evaluate(mode, params, scene=None):
    stamp = params['resume_from']
    if not is_stamp(stamp):
        print('Invalid resume folder')
        return
    log_dir, ckpt_dir, root = run_dirs(stamp)
    params.update(log_dir=log_dir, ckpt_dir=ckpt_dir, results_dir=os.path.join(root, RESULT_DIRS[mode]))
    Config.set_from_dict(params)
    print('Launching %s from checkpoint: %s' % ({'val': 'validation', 'test': 'testing', 'inference': 'inference',
                                                 'scene': 'scene colorization'}[mode], stamp))
    if mode == 'val':
        main_procedure.validation(**params)
    elif mode == 'test':
        main_procedure.test()
    elif mode == 'scene':
        return main_procedure.scene(params['instruction'], **scene)
    else:
        main_procedure.inference(params['infer_name'], params['instruction'])


def scene_arguments(args):
    """The checked arguments of --mode scene beside the instruction -> what main_procedure.scene takes."""
    if args.resume_from == '':
        raise ValueError('--mode scene needs --resume_from <stamp>: the run whose snapshot colours the instances')
    if args.image_id is None or args.inst_indices is None or args.instruction == '':
        raise ValueError("--mode scene needs --image_id <id>, --inst_indices <k,k,...> and --instruction '<text>'")
    try:
        indices = [int(k) for k in args.inst_indices.split(',')]
    except ValueError:
        raise ValueError('--inst_indices %r: comma-separated instance numbers, e.g. 7,8' % args.inst_indices)
    if not indices or min(indices) < 0:
        raise ValueError('--inst_indices %r: at least one instance, none negative' % args.inst_indices)
    if args.scene_size < 1:
        raise ValueError('--scene_size %d: a scene has at least one pixel' % args.scene_size)
    return dict(scene_dir=args.scene_dir, scene_size=args.scene_size, image_id=args.image_id, inst_indices=indices,
                previous_image=args.previous_image, noise_seed=args.noise_seed)


def main(argv=None):
    args = build_parser().parse_args(argv)
    params = {key: getattr(args, name) for name, _s, _t, _d, _c, key, _h in FLAGS}
    from sketchyscenecolorization_amd import preview
    preview.checked_count(args.val_preview, args.val_freq, args.mode, freq_flag='--val_freq (-vf)')
    from sketchyscenecolorization_amd import metrics
    metrics.checked_color_flag(args.color_metrics, args.metrics, args.val_freq, args.mode, scored_modes=('val', 'test'),
                               metrics_flag='--metrics (-mt)', freq_flag='--val_freq (-vf)')
    if args.mode == 'scene':
        return evaluate('scene', params, scene_arguments(args))
    given = [name for name, _s, _t, default, _h in SCENE_FLAGS if getattr(args, name) != default]
    if given:
        raise ValueError('--%s belongs to --mode scene, this is --mode %s' % (', --'.join(given), args.mode))
    if args.mode != 'train':
        if args.mode == 'inference':
            assert args.infer_name != '' and args.instruction != '', '--infer_name and --instruction are required'
        return evaluate(args.mode, params)
    # -gpu N without a launcher: the towers are processes here, so the command starts itself once per GPU
    from sketchyscenecolorization_amd.dist_utils import launch_towers
    # a programmatic caller's explicit argv is what the ranks must see, under the host script (which may wrap this module)
    import sys
    rc = launch_towers(args.num_gpu, None if argv is None else [sys.argv[0]] + list(argv))
    if rc is not None:
        if rc != 0:
            raise SystemExit(rc)
        return
    status, stamp = start_or_resume_training(params)
    while status == -1:         # a NaN loss ends train() with -1: continue from the last snapshot
        print('Training ended with status -1. Restarting..')
        params['resume_from'] = stamp
        status, stamp = start_or_resume_training(params)


if __name__ == '__main__':
    main()
