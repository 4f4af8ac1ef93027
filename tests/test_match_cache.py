"""The host side of the matcher's device scene cache (sketchyscenecolorization_amd/match_cache.py, match_main.py --mode train
--scene_cache), without a GPU: the byte arithmetic, the refusal and what it says, the order of the distinct scenes, the flag."""
import os

import pytest

import match_eval_oracle as EO
from sketchyscenecolorization_amd import match_cache as C, match_eval, matching as M, tf_checkpoint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = os.path.join(ROOT, 'tests', 'golden', 'match', 'vocab.txt')
SMALL = dict(size=64, units=(1, 1, 1, 1), filters=(8, 16, 32, 64, 128))


def test_cache_bytes_are_the_figures_of_the_design():
    assert C.cache_bytes(1, 768) == (2359296, 0)
    assert C.cache_bytes(1, 768, 2048) == (2359296, 96 * 96 * 2048 * 4) and 96 * 96 * 2048 * 4 == 75497472
    scenes, feats = C.cache_bytes(1337, 768, 2048)
    assert scenes == 1337 * 768 * 768 * 4 and round(scenes / 1e9, 1) == 3.2
    assert feats == 1337 * 75497472 and round(feats / 1e9, 1) == 100.9
    assert C.cache_bytes(2, 64, 128) == (2 * 64 * 64 * 4, 2 * 8 * 8 * 128 * 4)
    assert C.cache_bytes(0, 64, 128) == (0, 0)


def test_budget_is_half_of_what_was_free_and_the_refusal_names_bytes_and_remedy():
    C.check_budget(500, 0, 1000)
    C.check_budget(200, 300, 1000)
    C.check_budget(200, 300, 1001)                      # half of an odd number, rounded down: 500
    with pytest.raises(ValueError) as e:
        C.check_budget(501, 0, 1000)
    assert '501 bytes' in str(e.value) and '1000 bytes free' in str(e.value) and '--scene_cache off' in str(e.value)
    with pytest.raises(ValueError) as e:
        C.check_budget(200, 301, 1000)
    assert '301 bytes' in str(e.value) and '200 bytes' in str(e.value) and '1000 bytes free' in str(e.value)
    assert '--scene_cache device' in str(e.value) and '--scene_cache off' not in str(e.value)
    with pytest.raises(ValueError, match='--scene_cache off'):          # the scenes alone do not fit: that is the remedy named
        C.check_budget(501, 301, 1000)
    with pytest.raises(ValueError, match='--val_scenes'):
        C.check_budget(501, 0, 1000, remedy_scenes='score fewer scenes (--val_scenes N)')
    # the whole train split with its features does not fit beside 288 GB free, the scenes alone do
    scenes, feats = C.cache_bytes(1337, 768, 2048)
    C.check_budget(scenes, feats, 288 << 30)
    with pytest.raises(ValueError, match='--scene_cache device'):
        C.check_budget(scenes, feats, 192 << 30)
    C.check_budget(scenes, 0, 192 << 30)


def test_distinct_scenes_keep_the_order_of_their_first_appearance():
    scenes = [('12', None), ('11', None), ('12', None), ('7', None), ('11', None)]
    ids, index = C.distinct_scenes(scenes)
    assert ids == ['12', '11', '7'] and index == {'12': 0, '11': 1, '7': 2}
    assert C.distinct_scenes([]) == ([], {})


def test_distinct_scenes_of_the_training_tuples(tmp_path):
    from sketchyscenecolorization_amd import match_train
    flags = EO.write_split(str(tmp_path), 'train')
    scenes = match_eval.read_captions(flags[3], 'train')
    tuples = match_train.training_tuples(scenes)
    assert len(tuples) == 6
    ids, index = C.distinct_scenes([(t[0], None) for t in tuples])
    assert ids == ['11', '12'] and index == {'11': 0, '12': 1}
    assert C.distinct_scenes(scenes)[0] == ids


def test_scene_cache_flag(tmp_path):
    import match_main
    d = match_main.build_parser().parse_args([])
    assert (d.scene_cache, d.val_freq, d.val_scenes) == ('off', 0, 0)
    cfg = M.MatchConfig(**SMALL)
    backbone = str(tmp_path / 'backbone-1')
    tf_checkpoint.write_checkpoint(backbone, {k: v for k, v in M.random_variables(cfg, 0).items() if k.startswith('ResNet/')})
    flags = EO.write_split(str(tmp_path), 'train')[:4]
    snaps, logs = str(tmp_path / 'snapshots'), str(tmp_path / 'log')
    good = ['--mode', 'train', '--backbone_snapshot', backbone, '--vocab_file', VOCAB, '--scene_size', '64', '--snapshot_root', snaps,
            '--log_root', logs, '--max_iteration', '4'] + flags
    for mode in ('off', 'device', 'features'):
        got = match_main.checked_train_arguments(match_main.build_parser().parse_args(good + ['--scene_cache', mode]))
        assert len(got) == 5 and len(got[2]) == 6
    for value in ('bogus', 'host', 'Device', ''):
        with pytest.raises(ValueError, match='scene_cache'):
            match_main.main(good + ['--scene_cache', value])
        assert not os.path.exists(snaps) and not os.path.exists(logs)
