#!/usr/bin/env python
"""Colour a scene sketch one instruction at a time (the reference's sketchyscene_colorization_main.py, with its flags, short
forms and defaults): an instruction that names a category goes to the instance matcher and the instance generator, any other to
the background generator; every result is recorded, and the last one can be taken back.

    python sketchyscene_colorization_main.py --image_id 9996 --instruction 'the bus on the left is yellow with blue windows'
    python sketchyscene_colorization_main.py --image_id 9996 --instruction 'the sky is pink and the ground is yellow'
    python sketchyscene_colorization_main.py --image_id 9996 --command withdraw
    python sketchyscene_colorization_main.py --image_id 9996 --script turns.txt

<results_base_dir>/results/<id>/ receives <id>_<k>.png for the k-th instruction, <id>_fg.png beside a background turn and the
report <id>_<k>.json (what was matched, the processed text, how many pixels changed per instance);
<results_base_dir>/update_records/<id>_records.json is the reference's record file, byte for byte
(sketchyscenecolorization_amd/scene_records.py).  --script FILE runs a file of turns -- one instruction per line, or the single
word ``withdraw``; blank lines and lines that start with # are skipped -- in one process on one SceneSession
(sketchyscenecolorization_amd/scene_session.py): the three networks are loaded once and the scene stays on
the device.  The snapshot roots are directories: the matcher's holds a TensorFlow checkpoint, the two generators' a snapshot of
obj_colorization_main.py / bg_colorization_main.py or a TensorFlow checkpoint.  Every bad argument and every missing file is a
ValueError before any weight is read or anything is written; --command withdraw loads no model.
"""
import argparse
import os

# the reference's flags (sketchyscene_colorization_main.py:61-97): (long, short, type, default, choices, help)
FLAGS = [
    ('command', 'c', str, 'color', ['color', 'withdraw'], "choose a command from 'color' or 'withdraw'"),
    ('image_id', 'id', int, -1, None, 'choose an image.'),
    ('instruction', 'it', str, '', None, 'the input instruction'),
    ('data_base_dir', 'dbd', str, 'examples', None, 'the base dir of examples'),
    ('results_base_dir', 'rbd', str, 'outputs', None, 'the dir of results'),
    ('match_snapshot_root', 'msr', str, 'Instance_Matching/outputs/snapshots', None, 'the dir of instance matching models'),
    ('match_vocab_path', 'mvp', str, 'Instance_Matching/data/vocab.txt', None, 'the instance matching vocabulary'),
    ('match_vocab_size', 'mvs', int, 76, None, 'vocab size of matching'),
    ('match_max_len', 'ml', int, 15, None, 'max sentence length of matching'),
    ('fgcolor_snapshot_root', 'fgsr', str, 'Foreground_Instance_Colorization/outputs/2019-00-00-00-00-00/snapshot', None,
     'the dir of foreground colorization models'),
    ('fgcolor_vocab_path', 'fgvp', str, 'Foreground_Instance_Colorization/data/vocab.txt', None,
     'the foreground colorization vocabulary'),
    ('fgcolor_vocab_size', 'fgvs', int, 58, None, 'vocab size of fg colorization'),
    ('fgcolor_max_len', 'fgl', int, 15, None, 'max sentence length of fg colorization'),
    ('bg_snapshot_root', 'bgsr', str, 'Background_Colorization/outputs/2019-00-00-00-00-00/snapshot', None,
     'the dir of background colorization models'),
    ('bg_vocab_path', 'bgvp', str, 'Background_Colorization/data/bg_vocab.txt', None, 'the background colorization vocabulary'),
    ('bg_vocab_size', 'bgvs', int, 18, None, 'vocab size of bg colorization'),
    ('bg_max_len', 'bgl', int, 8, None, 'max sentence length of bg colorization'),
]
# this project's own: (long, type, default, choices, help); the defaults are what the reference has built in
OWN_FLAGS = [
    ('scene_size', int, 768, None, 'square size of the scene (the inner mask has it, the sketch is brought to it)'),
    ('fgcolor_image_size', int, 192, [64, 192], 'the size the instance generator was trained at'),
    ('fgcolor_block_type', str, 'MRU', ['MRU', 'Pix2Pix', 'Residual'], 'the network family of the instance generator'),
    ('match_weights', str, 'deeplab', None, "the matcher's backbone: 'deeplab' or 'segnet' (match_main.py --weights)"),
    ('match_use_attn', int, 0, None, "1: the matcher's head with word attention (match_main.py --use_attn)"),
    ('color_gradient', int, 1, [0, 1], '1 = lighten the sky towards the top after a background turn (add_color_gradient)'),
    ('noise_seed', int, -1, None, '-1: noise drawn on the device; n >= 0: the p-th matched instance of a turn gets '
                                  'torch.randn(1, 256, generator=torch.Generator().manual_seed(n + p))'),
    ('script', str, '', None, "a file of turns for one process: an instruction per line, or the word 'withdraw'; blank lines "
                              'and lines that start with # are skipped'),
]
SCENE_FILES = (('sketches', '%s.png'), ('inner_masks', '%s.mat'), ('seg_data', '%s_datas.npz'))


def build_parser():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    for name, short, typ, default, choices, text in FLAGS:
        p.add_argument('--' + name, '-' + short, type=typ, default=default, choices=choices, help=text)
    for name, typ, default, choices, text in OWN_FLAGS:
        p.add_argument('--' + name, type=typ, default=default, choices=choices, help=text)
    return p


def parse_script(lines):
    """The lines of a --script file -> [('color', instruction) | ('withdraw', None)]."""
    turns = []
    for line in lines:
        line = line.strip()
        if line == '' or line.startswith('#'):
            continue
        turns.append(('withdraw', None) if line == 'withdraw' else ('color', line))
    return turns


def _snapshot_named(root, flag):
    """The file that <root>/checkpoint names (a snapshot of this project, or a TensorFlow checkpoint prefix) -> its path."""
    index = os.path.join(root, 'checkpoint')
    if not os.path.isfile(index):
        raise ValueError('--%s %r: no checkpoint file in it' % (flag, root))
    with open(index) as fp:
        line = fp.readline()
    if '"' not in line:
        raise ValueError('--%s %r: its checkpoint file names no snapshot' % (flag, root))
    path = os.path.join(root, os.path.basename(line.split('"')[1]))
    if not (os.path.isfile(path) or os.path.isfile(path + '.index')):
        raise ValueError('--%s %r: its checkpoint file names %s, which is not there' % (flag, root, os.path.basename(path)))
    tail = os.path.basename(path).rsplit('-', 1)
    if len(tail) != 2 or not tail[1].isdigit():
        raise ValueError('--%s %r: the snapshot %s carries no step number (<name>-<step>)' % (flag, root, os.path.basename(path)))
    return path


def _generator_vocab(path, size, flag):
    from sketchyscenecolorization_amd.data_processing.text_processing import load_vocab_dict_from_file
    if not os.path.isfile(path):
        raise ValueError('--%s_vocab_path %r: no such file' % (flag, path))
    vocab = load_vocab_dict_from_file(path)
    if not vocab or max(vocab.values()) >= size:
        raise ValueError('--%s_vocab_path %r holds %d words, --%s_vocab_size is %d' % (flag, path, len(vocab), flag, size))
    return vocab


def checked_withdraw(args):
    """--command withdraw: ValueError without an image or without a record; nothing is imported that needs the device."""
    from sketchyscenecolorization_amd import scene_records
    if args.image_id == -1:
        raise ValueError('--image_id <id> is needed')
    if args.script != '':
        raise ValueError("--command withdraw takes no --script: a script's own 'withdraw' lines run under --command color")
    if not os.path.isfile(scene_records.records_path(args.image_id, args.results_base_dir)):
        raise ValueError('No record to withdraw for image %s under %s' % (args.image_id, args.results_base_dir))


def checked_arguments(args, match_config=None):
    """--command color: every bad argument and every missing file is a ValueError here, before any weight is read or anything is
    written.  -> (the turns, the matcher's config and snapshot prefix, {'fg', 'bg'} snapshot paths, the three vocabularies)."""
    if args.image_id == -1:
        raise ValueError('--image_id <id> is needed')
    if args.script != '' and args.instruction != '':
        raise ValueError('--script and --instruction exclude each other: the instructions are the lines of the script')
    if args.script == '' and args.instruction == '':
        raise ValueError("--command color needs --instruction '<text>' or --script <file>")
    if args.script != '':
        if not os.path.isfile(args.script):
            raise ValueError('--script %r: no such file' % args.script)
        with open(args.script) as fp:
            turns = parse_script(fp.readlines())
        if not turns:
            raise ValueError('--script %r holds no turn' % args.script)
    else:
        turns = [('color', args.instruction)]
    if args.results_base_dir == '':
        raise ValueError('--results_base_dir is empty')
    if args.scene_size < 16 or args.scene_size > 4096:
        raise ValueError('--scene_size %d: from 16 (the sky colour is sought in rows 5 and 6) to 4096' % args.scene_size)
    if args.match_max_len < 1 or args.fgcolor_max_len < 1 or args.bg_max_len < 1:
        raise ValueError('--match_max_len %d, --fgcolor_max_len %d, --bg_max_len %d: each at least one word'
                         % (args.match_max_len, args.fgcolor_max_len, args.bg_max_len))
    for sub, name in SCENE_FILES:
        if not os.path.isfile(os.path.join(args.data_base_dir, sub, name % args.image_id)):
            raise ValueError('--data_base_dir %r has no %s/%s' % (args.data_base_dir, sub, name % args.image_id))
    import match_main
    from types import SimpleNamespace
    cfg, match_vocab = match_main.checked_model(SimpleNamespace(
        use_attn=args.match_use_attn, weights=args.match_weights, text_len=args.match_max_len, scene_size=args.scene_size,
        vocab_size=args.match_vocab_size, vocab_file=args.match_vocab_path))
    if match_config is not None:
        cfg = match_main.agreed_config(match_config, cfg)
    vocabs = {'match': match_vocab, 'fg': _generator_vocab(args.fgcolor_vocab_path, args.fgcolor_vocab_size, 'fgcolor'),
              'bg': _generator_vocab(args.bg_vocab_path, args.bg_vocab_size, 'bg')}
    try:
        prefix = match_main.checked_snapshot_variables(args.match_snapshot_root, cfg)
    except ValueError as e:
        raise ValueError('--match_snapshot_root: %s' % e)
    snapshots = {'fg': _snapshot_named(args.fgcolor_snapshot_root, 'fgcolor_snapshot_root'),
                 'bg': _snapshot_named(args.bg_snapshot_root, 'bg_snapshot_root')}
    return turns, cfg, prefix, snapshots, vocabs


def load_models(args, cfg, prefix, snapshots):
    """The three networks, each loaded once.  What they need is added up first and refused as a ValueError when it is more than
    half of what is free on the device."""
    import torch
    import bg_colorization_main
    import match_main
    from sketchyscenecolorization_amd import scene_session
    from sketchyscenecolorization_amd.bg_colorization import BGTrainer
    from sketchyscenecolorization_amd.obj_lib import main_procedure, models_collection as models
    need = scene_session.required_bytes(cfg, args.fgcolor_block_type, args.fgcolor_vocab_size, args.fgcolor_image_size,
                                        args.bg_vocab_size, args.scene_size)
    total = scene_session.check_budget(need, torch.cuda.mem_get_info()[0])
    print('scene session: %d bytes of weights and scene state on the device' % total)
    matcher = match_main.reserved_model(cfg)
    matcher.load_tf_checkpoint(prefix)
    print('loaded', prefix)
    models.reset_default_graph()                # as obj_lib/main_procedure.scene builds its tower
    fg = models.get_trainer(args.fgcolor_block_type, args.fgcolor_vocab_size, args.fgcolor_image_size)
    path = main_procedure.latest_checkpoint(args.fgcolor_snapshot_root)
    print('Restore trained model:', path)
    main_procedure.restore_checkpoint(fg.store, path)
    fg.G.lstm_hybrid = True
    bg = BGTrainer(image_size=args.scene_size, vocab_size=args.bg_vocab_size)      # as bg_colorization_main's scene mode
    print('iter_from', bg_colorization_main.load_checkpoint(bg, args.bg_snapshot_root))
    return matcher, fg, bg


def turn_line(report):
    changed = report['changed']
    return '%s matched_inst_indices %s result %s changed background %d instances %d' % (
        report['colorization_type'], ','.join(str(k) for k in report['matched_inst_indices']) or '-', report['result_name'],
        changed['background'], sum(changed['instances'].values()))


def main(argv=None, match_config=None):
    """``match_config``: a MatchConfig other than the released model's (the tests' small models); its size, vocabulary size and
    text length must be the flags'."""
    args = build_parser().parse_args(argv)
    if args.command == 'withdraw':
        checked_withdraw(args)
        from sketchyscenecolorization_amd import scene_records
        left = scene_records.withdraw(args.image_id, args.results_base_dir)
        print('withdrawn: %d editing records left' % len(left))
        return left
    turns, cfg, prefix, snapshots, vocabs = checked_arguments(args, match_config)
    from sketchyscenecolorization_amd import fg_scene, matching, scene_session
    scene = fg_scene.load_instances(args.data_base_dir, args.image_id, args.scene_size)
    matching.pack_masks(scene['boxes'], scene['masks'], args.scene_size)     # a bad box is refused before the weights are read
    matcher, fg, bg = load_models(args, cfg, prefix, snapshots)
    session = scene_session.SceneSession(matcher, fg, bg, vocabs, args.data_base_dir, args.results_base_dir, args.scene_size,
                                         fg_max_len=args.fgcolor_max_len, bg_max_len=args.bg_max_len,
                                         color_gradient=bool(args.color_gradient), noise_seed=args.noise_seed)
    session.open(args.image_id)
    reports = []
    for op, text in turns:
        if op == 'withdraw':
            print('withdrawn: %d editing records left' % len(session.withdraw()))
        else:
            reports.append(session.color(text))
            print(turn_line(reports[-1]))
    session.close()
    return reports


if __name__ == '__main__':
    main()
