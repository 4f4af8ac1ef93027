"""bg_colorization_main.py --scene_cache device / --recolor 1, the host side (no GPU): the flags, the colour augmentation against
the files the reference's own generator wrote (tests/golden/bg_aug/, made by tests/golden/make_bg_aug_goldens.py), the cache
builder on 'cpu' and what the command line feeds a (fake) trainer per step."""
import json
import os
import random
import shutil
import types

import numpy as np
import pytest
import torch
from PIL import Image

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'bg_aug')


def _records():
    with open(os.path.join(FIX, 'captions', 'train.json')) as fp:
        return json.load(fp)


def _png(kind, name):
    return np.array(Image.open(os.path.join(FIX, kind, 'train', name)).convert('RGB'), dtype=np.uint8)


class _Reached(Exception):
    pass


def test_flags_and_their_defaults(tmp_path, monkeypatch):
    import bg_colorization_main as bgcli
    from sketchyscenecolorization_amd import bg_colorization
    args = bgcli.build_parser().parse_args([])
    assert args.scene_cache == 'off' and args.recolor == 0
    args = bgcli.build_parser().parse_args(['--scene_cache', 'device', '--recolor', '1'])
    assert args.scene_cache == 'device' and args.recolor == 1
    with pytest.raises(SystemExit):
        bgcli.build_parser().parse_args(['--scene_cache', 'host'])
    built = []

    class FakeTrainer(object):
        def __init__(self, **kw):
            built.append(kw)
            raise _Reached()

    monkeypatch.setattr(bg_colorization, 'BGTrainer', FakeTrainer)
    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError, match='scene_cache device'):
        bgcli.main(['--mode', 'train', '--recolor', '1', '--image_size', '32', '--max_steps', '2'])
    assert not built, 'the trainer was built before --recolor 1 without the cache was refused'
    with pytest.raises(_Reached):
        bgcli.main(['--mode', 'train', '--scene_cache', 'device', '--recolor', '1', '--image_size', '32', '--max_steps', '2'])
    assert len(built) == 1


def test_recolour_formula_caption_and_palette_are_the_reference_generators():
    """Every augmented background the reference wrote is where(seg == 128, sky, where(seg == 255, ground, base)) of its base
    record, byte for byte; its caption is bg_palette.caption of the pair; the colours in the files are the table's."""
    from sketchyscenecolorization_amd.data_processing import bg_palette as pal
    recs = _records()
    assert len(recs) == 8
    assert len(pal.PAIRS) == 50 and len(set(pal.PAIRS)) == 50 and all(s != g for s, g in pal.PAIRS)
    assert pal.PAIRS[0] == ('blue', 'yellow') and pal.PAIRS[1] == pal.BASE_PAIR and pal.PAIRS[-1] == ('gray', 'brown')
    assert set(pal.COLOR_MAP) == set(pal.SKY_COLOR) and set(pal.GROUND_COLOR) < set(pal.SKY_COLOR)
    seen_aug = 0
    for rec in recs:
        words = rec['color_text'].split()
        sky, ground = words[3], words[-1]
        assert (sky, ground) in pal.PAIRS and pal.caption(sky, ground) == rec['color_text']
        base, seg = _png('background', rec['fg_name']), _png('segment', rec['fg_name'])[:, :, 0]
        want = _png('background', rec['bg_name'])
        assert set(np.unique(seg)) == {0, 128, 255}
        got = pal.recolor(base, seg, sky, ground)
        assert np.array_equal(got, want), rec
        # the explicit where-formula and the 8-byte record of the kernel say the same
        r8 = pal.recolor_record(sky, ground)
        assert r8.dtype == np.uint8 and r8.shape == (8,) and r8[0] == 1 and r8[7] == 0
        where = np.where((seg == 128)[..., None], r8[1:4], np.where((seg == 255)[..., None], r8[4:7], base))
        assert np.array_equal(where, want)
        # the palette: the sky and ground pixels of the file are exactly the table's colours
        assert np.all(want[seg == 128] == np.array(pal.COLOR_MAP[sky], np.uint8))
        assert np.all(want[seg == 255] == np.array(pal.COLOR_MAP[ground], np.uint8))
        if rec['bg_name'] == rec['fg_name']:
            assert (sky, ground) == pal.BASE_PAIR
            # the segment map is *defined* by the base colours: background by the mask, and blue / green
            mask = _png('inner_mask', rec['fg_name'])[:, :, 0]
            blue = (base == np.array(pal.COLOR_MAP['blue'], np.uint8)).all(2)
            green = (base == np.array(pal.COLOR_MAP['green'], np.uint8)).all(2)
            assert np.array_equal(seg == 128, (mask == 255) & blue) and np.array_equal(seg == 255, (mask == 255) & green)
            assert ((seg == 0) & (mask == 255)).any() and ((mask == 0) & blue).any() and ((mask == 100) & blue).any()
        else:
            seen_aug += 1
            assert not np.array_equal(want, base)
    assert seen_aug == 6
    with open(os.path.join(FIX, 'bg_vocab.txt')) as fp:
        vocab = [w.strip() for w in fp]
    assert len(vocab) == 18 and set(pal.SKY_COLOR) < set(vocab)


def _dataset(tmp_path, size=12):
    """The fixture as a dataset of the command line: every png cut to its top-left size x size corner, because the loader
    takes square scenes of one size and the fixture's two scenes are 16 x 16 and 12 x 20.  All 12 files stay distinct."""
    base = tmp_path / 'data'
    for kind in ('foreground', 'background', 'segment'):
        os.makedirs(str(base / kind / 'train'))
        for name in sorted(os.listdir(os.path.join(FIX, kind, 'train'))):
            im = Image.open(os.path.join(FIX, kind, 'train', name))
            im.crop((0, 0, size, size)).save(str(base / kind / 'train' / name))
    os.makedirs(str(base / 'captions'))
    shutil.copyfile(os.path.join(FIX, 'captions', 'train.json'), str(base / 'captions' / 'train.json'))
    shutil.copyfile(os.path.join(FIX, 'bg_vocab.txt'), str(base / 'bg_vocab.txt'))
    return {'image_size': size, 'text_len': 8, 'data_base_dir': str(base), 'mode': 'train', 'vocab_size': 18,
            'vocab_file': str(base / 'bg_vocab.txt')}


SEG_OF = np.array([0, 128, 255], np.uint8)


def test_scene_cache_holds_each_file_once(tmp_path):
    import bg_colorization_main as bgcli
    from sketchyscenecolorization_amd.scene_cache import SceneCache
    scenes = bgcli.Scenes(_dataset(tmp_path))
    cache = SceneCache(scenes, device='cpu')
    assert cache.fg.shape == (2, 12, 12, 3) and cache.bg.shape == (8, 12, 12, 3) and cache.seg.shape == (2, 12, 12)
    assert cache.fg.dtype == cache.bg.dtype == cache.seg.dtype == torch.uint8 and cache.fg.device.type == 'cpu'
    assert cache.nbytes == (2 + 8) * 144 * 3 + 2 * 144 and len(cache) == 8
    assert cache.slots.shape == (8, 3) and cache.slots.dtype == np.int32 and cache.tokens.shape == (8, 8)
    assert len({tuple(s) for s in cache.slots.tolist()}) == 8 and len(set(cache.slots[:, 1].tolist())) == 8
    for i in range(8):
        fg, bg, tok, lab, _, _ = scenes.get(i)
        sf, sb, ss = cache.slots[i]
        assert np.array_equal(cache.fg[sf].numpy(), fg[0]) and np.array_equal(cache.bg[sb].numpy(), bg[0])
        seg = cache.seg[ss].numpy()
        assert np.array_equal(np.where(seg == 128, 1, np.where(seg == 255, 2, 0)), lab[0])
        assert np.array_equal(cache.tokens[i], tok[0])
    # the base records only, renumbered in order
    base = SceneCache(scenes, device='cpu', keep=[0, 4])
    assert base.fg.shape[0] == base.bg.shape[0] == base.seg.shape[0] == 2 and len(base) == 2
    assert np.array_equal(base.bg[base.slots[1, 1]].numpy(), scenes.get(4)[1][0])


def test_scene_cache_refuses_a_segment_map_of_another_size(tmp_path):
    """The fixture as it is: scene_b is 12 rows x 20 columns.  Images are resized on load, segment maps are not."""
    import bg_colorization_main as bgcli
    from sketchyscenecolorization_amd.scene_cache import SceneCache
    p = _dataset(tmp_path)
    shutil.copyfile(os.path.join(FIX, 'segment', 'train', 'scene_b.png'), os.path.join(p['data_base_dir'], 'segment', 'train', 'scene_b.png'))
    with pytest.raises(ValueError, match=r'scene_b\.png is 20 x 12.*12 x 12'):
        SceneCache(bgcli.Scenes(p), device='cpu')


def test_scene_cache_of_the_synthetic_scenes():
    import bg_colorization_main as bgcli
    from sketchyscenecolorization_amd.scene_cache import SceneCache
    scenes = bgcli.Scenes({'image_size': 32, 'text_len': 8, 'data_base_dir': 'no_such_dir', 'mode': 'train', 'vocab_size': 18})
    cache = SceneCache(scenes, device='cpu')
    assert cache.fg.shape == (8, 32, 32, 3) and cache.seg.shape == (8, 32, 32) and len(cache) == 8
    for i in range(8):
        fg, bg, tok, lab, _, _ = scenes.get(i)
        assert cache.slots[i].tolist() == [i, i, i] and np.array_equal(cache.tokens[i], tok[0])
        assert np.array_equal(cache.fg[i].numpy(), fg[0]) and np.array_equal(cache.bg[i].numpy(), bg[0])
        assert np.array_equal(cache.seg[i].numpy(), SEG_OF[lab[0]])


def test_scene_cache_that_does_not_fit_is_refused(monkeypatch):
    """Asked for a device whose free memory is less than twice the cache, the builder stops before it allocates, with both
    numbers in the message."""
    import bg_colorization_main as bgcli
    from sketchyscenecolorization_amd import scene_cache
    scenes = bgcli.Scenes({'image_size': 32, 'text_len': 8, 'data_base_dir': 'no_such_dir', 'mode': 'train', 'vocab_size': 18})
    need = 8 * 32 * 32 * 7
    monkeypatch.setattr(torch.cuda, 'mem_get_info', lambda device=None: (2 * need - 2, 10 * need))
    monkeypatch.setattr(torch, 'empty', lambda *a, **k: pytest.fail('allocated although the cache does not fit'))
    with pytest.raises(RuntimeError) as e:
        scene_cache.SceneCache(scenes, device='cuda')
    assert str(need) in str(e.value) and str(2 * need - 2) in str(e.value)


def _fake_trainer(fed):
    class FakeScope(object):
        name = 'x'

    class FakeStore(object):
        generator = discriminator = FakeScope()

        def parameter_count(self, scope):
            return 0

    class FakeTrainer(object):
        def __init__(self, **kw):
            self.store, self.global_step = FakeStore(), 0
            self.losses = types.SimpleNamespace(device=torch.device('cpu'))      # where the command line puts the cache

        def train_step_u8(self, *a):
            raise AssertionError('--scene_cache device must not upload scenes per step')

        def train_step_cached(self, cache, slots, recolor, text):
            fed.append((cache, np.array(slots), None if recolor is None else np.array(recolor), np.array(text)))
            self.global_step += 1

    return FakeTrainer


def _gather(cache, slots):
    seg = cache.seg.numpy()[slots[:, 2]]
    return cache.fg.numpy()[slots[:, 0]], cache.bg.numpy()[slots[:, 1]], np.where(seg == 128, 1, np.where(seg == 255, 2, 0))


@pytest.mark.parametrize('dataset', ['synthetic', 'files'])
@pytest.mark.parametrize('nb', [1, 3])
def test_cli_feeds_the_scenes_of_the_uncached_run(tmp_path, monkeypatch, nb, dataset):
    """--scene_cache device --recolor 0: what the slots of a step gather from the cache is what Scenes.get returns for the
    draws of the uncached command line with the same seed -- over more steps than any staging ring has buffers."""
    import bg_colorization_main as bgcli
    from sketchyscenecolorization_amd import bg_colorization
    fed = []
    monkeypatch.setattr(bg_colorization, 'BGTrainer', _fake_trainer(fed))
    p = _dataset(tmp_path) if dataset == 'files' else {'image_size': 32, 'text_len': 8, 'data_base_dir': 'data', 'mode': 'train',
                                                        'vocab_size': 18, 'vocab_file': 'data/bg_vocab.txt'}
    monkeypatch.chdir(tmp_path)
    steps = 6
    random.seed(5)
    bgcli.main(['--mode', 'train', '--batch_size', str(nb), '--image_size', str(p['image_size']), '--max_steps', str(steps),
                '--save_freq', '0', '--progress_freq', '0', '--summary_freq', '0', '--scene_cache', 'device',
                '--data_base_dir', p['data_base_dir'], '--vocab_file', p['vocab_file']])
    random.seed(5)
    random.randint(0, 2 ** 31 - 1)      # the trainer's seed
    scenes = bgcli.Scenes(p)
    assert len(fed) == steps and len({id(f[0]) for f in fed}) == 1, 'one cache, built once'
    for cache, slots, recolor, tok in fed:
        want = [scenes.get(random.randint(0, len(scenes) - 1)) for _ in range(nb)]
        assert recolor is None and slots.shape == (nb, 3) and slots.dtype == np.int32 and tok.shape == (nb, 8)
        fg, bg, lab = _gather(cache, slots)
        for i, w in enumerate(want):
            assert np.array_equal(fg[i], w[0][0]) and np.array_equal(bg[i], w[1][0])
            assert np.array_equal(tok[i], w[2][0]) and np.array_equal(lab[i], w[3][0])


@pytest.mark.parametrize('nb', [1, 3])
def test_cli_recolor_draws_a_valid_pair_per_sample(tmp_path, monkeypatch, nb):
    """--recolor 1: the scenes are the base records, drawn by the same sequence of random.randint calls (one more at start-up
    seeds the pairs' own generator); every sample carries a valid pair, the tokens of its caption and the base background."""
    import bg_colorization_main as bgcli
    from sketchyscenecolorization_amd import bg_colorization
    from sketchyscenecolorization_amd.data_processing import bg_palette as pal
    from sketchyscenecolorization_amd.data_processing.text_processing import load_vocab_dict_from_file, preprocess_sentence
    fed = []
    monkeypatch.setattr(bg_colorization, 'BGTrainer', _fake_trainer(fed))
    p = _dataset(tmp_path)
    monkeypatch.chdir(tmp_path)
    steps = 6
    random.seed(11)
    bgcli.main(['--mode', 'train', '--batch_size', str(nb), '--image_size', '12', '--max_steps', str(steps), '--save_freq', '0',
                '--progress_freq', '0', '--summary_freq', '0', '--scene_cache', 'device', '--recolor', '1',
                '--data_base_dir', p['data_base_dir'], '--vocab_file', p['vocab_file']])
    random.seed(11)
    random.randint(0, 2 ** 31 - 1)      # the trainer's seed
    pair_rng = random.Random(random.randint(0, 2 ** 31 - 1))
    scenes = bgcli.Scenes(p)
    base = [0, 4]                       # the records with bg_name == fg_name
    vocab = load_vocab_dict_from_file(p['vocab_file'])
    by_rgb = {(1,) + pal.COLOR_MAP[s] + pal.COLOR_MAP[g] + (0,): (s, g) for s, g in pal.PAIRS}
    assert len(fed) == steps
    pairs_seen = set()
    for cache, slots, recolor, tok in fed:
        assert cache.bg.shape[0] == 2 and recolor.shape == (nb, 8) and recolor.dtype == np.uint8
        fg, bg, lab = _gather(cache, slots)
        for i in range(nb):
            w = scenes.get(base[random.randint(0, len(base) - 1)])
            assert np.array_equal(fg[i], w[0][0]) and np.array_equal(bg[i], w[1][0]) and np.array_equal(lab[i], w[3][0])
            sky, ground = by_rgb[tuple(recolor[i].tolist())]
            assert (sky, ground) == pal.PAIRS[pair_rng.randint(0, 49)]
            assert tok[i].tolist() == preprocess_sentence(pal.caption(sky, ground), vocab, 8)
            pairs_seen.add((sky, ground))
    assert len(pairs_seen) > 1
    # no base record: said so
    with open(os.path.join(p['data_base_dir'], 'captions', 'train.json'), 'w') as fp:
        json.dump([r for r in _records() if r['bg_name'] != r['fg_name']], fp)
    with pytest.raises(ValueError, match='base record'):
        bgcli.main(['--mode', 'train', '--image_size', '12', '--max_steps', '1', '--scene_cache', 'device', '--recolor', '1',
                    '--data_base_dir', p['data_base_dir'], '--vocab_file', p['vocab_file']])
