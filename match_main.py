"""Pick the instances of a user scene that an instruction speaks of (Pipeline_utils/fg_matching_utils.py::
build_instance_matching): the RMI matcher's forward pass and the choice by mask occupancy, on the device
(sketchyscenecolorization_amd/matching.py).

    python match_main.py --snapshot outputs/match_snapshot --image_id 77742204 --instruction 'the bus on the left is yellow'

prints one line ``matched_inst_indices 7,8`` -- what ``obj_colorization_main.py --mode scene ... --inst_indices`` takes -- and
writes <results_dir>/<id>/match.json and <id>_match.png (the prediction on the strokes, x 255)."""
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
]


def build_parser():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    for name, typ, default, text in FLAGS:
        p.add_argument('--' + name, type=typ, default=default, help=text)
    return p


def checked_arguments(args):
    """Every bad argument is a ValueError here, before anything is loaded or written.  -> (config, snapshot prefix, vocab)."""
    from sketchyscenecolorization_amd import matching
    if args.snapshot == '':
        raise ValueError('--snapshot <directory or checkpoint prefix> is needed: the matcher has no weights of its own')
    if args.image_id is None or args.image_id == '' or args.instruction == '':
        raise ValueError("--image_id <id> and --instruction '<text>' are needed")
    if args.text_len < 1:
        raise ValueError('--text_len %d: at least one word' % args.text_len)
    config = matching.MatchConfig(size=args.scene_size, vocab_size=args.vocab_size, max_len=args.text_len)
    if not matching.sentence_tokens(args.instruction):
        raise ValueError('--instruction %r holds no word' % args.instruction)
    if not os.path.isfile(args.vocab_file):
        raise ValueError('--vocab_file %r: no such file' % args.vocab_file)
    vocab = matching.load_vocab(args.vocab_file)
    if len(vocab) != args.vocab_size or matching.UNK not in vocab or matching.PAD not in vocab:
        raise ValueError('--vocab_file %r holds %d words, --vocab_size is %d; <unk> and <pad> must be among them'
                         % (args.vocab_file, len(vocab), args.vocab_size))
    prefix = matching.resolve_snapshot(args.snapshot)
    for sub, name in (('sketches', args.image_id + '.png'), ('inner_masks', args.image_id + '.mat'),
                      ('seg_data', args.image_id + '_datas.npz')):
        if not os.path.isfile(os.path.join(args.scene_dir, sub, name)):
            raise ValueError('--scene_dir %r has no %s/%s' % (args.scene_dir, sub, name))
    return config, prefix, vocab


def main(argv=None, config=None):
    """``config``: a MatchConfig other than the released model's (the tests' small models); its size, vocabulary size and
    text length must be the flags'."""
    args = build_parser().parse_args(argv)
    cfg, prefix, vocab = checked_arguments(args)
    if config is not None:
        if (config.size, config.vocab_size, config.max_len) != (cfg.size, cfg.vocab_size, cfg.max_len):
            raise ValueError('the given configuration and --scene_size / --vocab_size / --text_len disagree')
        cfg = config
    import numpy as np
    from PIL import Image
    from sketchyscenecolorization_amd import fg_scene, matching
    scene = fg_scene.load_instances(args.scene_dir, args.image_id, cfg.size)
    matching.pack_masks(scene['boxes'], scene['masks'], cfg.size)       # a bad box is refused before the weights are read
    model = matching.MatchModel(cfg)
    model.load_tf_checkpoint(prefix)
    matched, scores, info = matching.match_instances(model, scene, args.instruction, vocab)
    model.close()
    out_dir = os.path.join(args.results_dir, str(args.image_id))
    os.makedirs(out_dir, exist_ok=True)
    record = {'image_id': str(args.image_id), 'instruction': args.instruction, 'tokens': info['tokens'], 'seq_len': info['seq_len'],
              'matched_inst_indices': matched,
              'occupancy': [None if s != s else float(s) for s in scores.tolist()],
              'class_ids': [int(c) for c in np.asarray(scene['class_ids']).reshape(-1)], 'snapshot': prefix}
    with open(os.path.join(out_dir, 'match.json'), 'w') as f:
        json.dump(record, f, indent=1)
    Image.fromarray((info['predicts'] != 0).astype(np.uint8) * 255).save(os.path.join(out_dir, '%s_match.png' % args.image_id))
    print('matched_inst_indices ' + ','.join(str(k) for k in matched))
    return matched


if __name__ == '__main__':
    main()
