"""The matcher's device scene cache (sketchyscenecolorization_amd/match_cache.py, MatchTrainer.step's device-resident scene,
match_main.py --mode train --scene_cache): the entries against match_eval.load_ground_truth byte for byte, the areas against
np.bincount, the cached features against MatchModel.features bit for bit, three steps from each form of the scene argument to the
same parameters and Adam slots, and the command line in fresh processes: off, device and features write the same snapshots, also
across a resume that switches the mode.  The held-out pass that reads such a cache ends in hip.match_score (ssc_match_score),
tests/test_gpu_match_validation.py."""
import faulthandler
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import match_eval_oracle as EO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = os.path.join(ROOT, 'tests', 'golden', 'match', 'vocab.txt')
CHILD_LIMIT = 180
SMALL = dict(size=64, units=(1, 1, 1, 1), filters=(8, 16, 32, 64, 128))
NARROW = dict(v_emb=24, w_emb=24, w_rnn=40, m_rnn=20)


@pytest.fixture(autouse=True)
def _time_limit():
    """A test that hangs on the device ends the process (with every thread's traceback) instead of holding the card."""
    faulthandler.dump_traceback_later(400, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _second_scene_gets_other_labels(base, split):
    """Scene 12 with its rectangles at other places, so that a wrong gather shows in the lut and the areas, not only in the sketch."""
    import scipy.io
    gt = np.zeros((60, 60), np.uint8)
    for k, (y1, x1, y2, x2) in enumerate([(30, 30, 58, 58), (2, 2, 12, 40), (14, 2, 28, 20), (2, 44, 28, 58), (32, 2, 58, 26)]):
        gt[y1:y2, x1:x2] = (k + 1) * 5
    scipy.io.savemat(os.path.join(base, 'data', split, 'INSTANCE_GT', 'sample_12_instance.mat'), {'INSTANCE_GT': gt})


@pytest.fixture(scope='module')
def split(tmp_path_factory):
    """The synthetic train split, a loaded small model, and the reference arrays of both scenes (read once)."""
    from sketchyscenecolorization_amd import match_eval, matching as m
    base = str(tmp_path_factory.mktemp('match_cache'))
    flags = EO.write_split(base, 'train')
    _second_scene_gets_other_labels(base, 'train')
    scenes = match_eval.read_captions(flags[3], 'train')
    cfg = m.MatchConfig(**dict(SMALL, **NARROW))
    variables = m.random_variables(cfg, 17)
    gts = [match_eval.load_ground_truth(flags[1], 'train', image_id, 64) for image_id, _p in scenes]
    assert not np.array_equal(gts[0]['labels'], gts[1]['labels']) and not np.array_equal(gts[0]['sketch'], gts[1]['sketch'])
    return dict(base=base, data=flags[1], scenes=scenes, cfg=cfg, variables=variables, gts=gts)


def _model(split):
    from sketchyscenecolorization_amd import matching as m
    model = m.MatchModel(split['cfg'])
    model.load_dict(split['variables'])
    return model


def test_entries_are_the_readers_arrays(split):
    from sketchyscenecolorization_amd import match_cache
    model = _model(split)
    doubled = split['scenes'] + split['scenes'][::-1]                    # every scene twice: read once, in the order of appearance
    cache = match_cache.MatchSceneCache(doubled, split['data'], 'train', 64, 'cuda', features=model)
    assert len(cache) == 2 and cache.ids == ['11', '12'] and cache.index == {'11': 0, '12': 1}
    assert (cache.scene_bytes, cache.feature_bytes) == match_cache.cache_bytes(2, 64, 128) and cache.nbytes == 2 * 64 * 64 * 4 + 2 * 8 * 8 * 128 * 4
    assert cache.sketch.dtype == cache.labels.dtype == torch.uint8 and cache.sketch.is_cuda and cache.feat.dtype == torch.float32
    assert tuple(cache.sketch.shape) == (2, 64, 64, 3) and tuple(cache.labels.shape) == (2, 64, 64) and tuple(cache.feat.shape) == (2, 8, 8, 128)
    assert cache.area.dtype == np.int64 and cache.area.shape == (2, 256) and cache.n_inst.dtype == np.int64 and cache.n_inst.tolist() == [5, 5]
    for i, gt in enumerate(split['gts']):
        e = cache.entry(i)
        assert sorted(e) == ['feat_d', 'image_id', 'labels_d', 'n_inst', 'sketch_d'] and e['image_id'] == gt['image_id']
        assert np.array_equal(e['sketch_d'].cpu().numpy(), gt['sketch']) and np.array_equal(e['labels_d'].cpu().numpy(), gt['labels'])
        assert e['sketch_d'].data_ptr() % 16 == 0 and e['labels_d'].data_ptr() % 16 == 0 and e['feat_d'].data_ptr() % 16 == 0
        assert np.array_equal(cache.area[i], np.bincount(gt['labels'].reshape(-1), minlength=256))
        assert e['n_inst'] == gt['n_inst']
        feat, _stroke = model.features(gt['sketch'])
        assert tuple(e['feat_d'].shape) == tuple(feat.shape) == (1, 8, 8, 128) and float(feat.abs().max()) > 0
        assert torch.equal(e['feat_d'], feat)
        assert cache.entry(gt['image_id'])['sketch_d'].data_ptr() == e['sketch_d'].data_ptr()
    assert not np.array_equal(cache.area[0], cache.area[1]) and not torch.equal(cache.feat[0], cache.feat[1])
    plain = match_cache.MatchSceneCache(split['scenes'], split['data'], 'train', 64, 'cuda')
    assert plain.feat is None and plain.feature_bytes == 0 and sorted(plain.entry(1)) == ['image_id', 'labels_d', 'n_inst', 'sketch_d']
    assert torch.equal(plain.sketch, cache.sketch) and torch.equal(plain.labels, cache.labels) and np.array_equal(plain.area, cache.area)
    model.close()


def test_cache_refusals(split):
    from sketchyscenecolorization_amd import match_cache, matching as m
    free = torch.cuda.mem_get_info()[0]
    with pytest.raises(ValueError, match='no such file'):              # the reader's own refusal
        match_cache.MatchSceneCache([('404', None)], split['data'], 'train', 64, 'cuda')
    with pytest.raises(ValueError, match='--scene_cache off') as e:    # other caches beside it that leave no room
        match_cache.MatchSceneCache(split['scenes'], split['data'], 'train', 64, 'cuda', beside=free)
    assert ' bytes free' in str(e.value)
    unloaded = m.MatchModel(split['cfg'])
    with pytest.raises(RuntimeError, match='weights'):
        match_cache.MatchSceneCache(split['scenes'], split['data'], 'train', 64, 'cuda', features=unloaded)
    unloaded.close()


def _state(trainer):
    return [t.clone() for t in (trainer.params, trainer.adam_m, trainer.adam_v)]


def test_three_forms_of_the_scene_argument_train_the_same_bits(split):
    """Three steps over both scenes from host arrays, from the cached sketch and labels, and from the cached features too."""
    from sketchyscenecolorization_amd import match_cache, match_eval, match_train as T, matching as m
    vocab = m.load_vocab(VOCAB)
    tuples = T.training_tuples(split['scenes'])
    order = [0, 4, 2]                                                   # scene 11, scene 12, scene 11
    states, losses = {}, {}
    for form in ('host', 'device', 'features'):
        model = _model(split)
        trainer = T.MatchTrainer(model)
        cache = None if form == 'host' else match_cache.MatchSceneCache(split['scenes'], split['data'], 'train', 64, 'cuda',
                                                                        features=model if form == 'features' else None)
        for k in order:
            image_id, caption, inst_indices = tuples[k]
            i = [s[0] for s in split['scenes']].index(image_id)
            gt = split['gts'][i]
            area = np.bincount(gt['labels'].reshape(-1), minlength=256) if cache is None else cache.area[i]
            lut = T.caption_lut(match_eval.caption_labels(image_id, inst_indices, gt['n_inst'], area))
            indices, seq_len = m.preprocess_sentence(caption, vocab, split['cfg'].max_len)
            scene = gt if cache is None else cache.entry(image_id)
            assert ('feat_d' in scene) == (form == 'features')
            trainer.step(scene, lut, indices, seq_len, 1e-3)
        states[form], losses[form] = _state(trainer), trainer.last_loss()
        model.close()
    assert float((states['host'][0] - _model_params(split)).abs().max()) > 0
    for form in ('device', 'features'):
        assert losses[form] == losses['host']
        for a, b in zip(states[form], states['host']):
            assert torch.equal(a, b), form


def _model_params(split):
    from sketchyscenecolorization_amd import match_train as T
    model = _model(split)
    p = T.MatchTrainer(model).params.clone()
    model.close()
    return p


def test_step_refuses_a_resident_scene_of_another_shape(split):
    from sketchyscenecolorization_amd import match_train as T
    model = _model(split)
    trainer = T.MatchTrainer(model)
    lut, idx = np.zeros(256, np.uint8), np.zeros(15, np.int64)
    good = {'sketch_d': torch.zeros((64, 64, 3), dtype=torch.uint8, device='cuda'),
            'labels_d': torch.zeros((64, 64), dtype=torch.uint8, device='cuda')}
    for key, bad in (('sketch_d', torch.zeros((64, 64, 4), dtype=torch.uint8, device='cuda')),
                     ('labels_d', torch.zeros((64, 64), dtype=torch.int32, device='cuda')),
                     ('sketch_d', torch.zeros((64, 64, 3), dtype=torch.uint8)),
                     ('feat_d', torch.zeros((8, 8, 128), device='cuda'))):
        with pytest.raises(ValueError, match=key):
            trainer.step(dict(good, **{key: bad}), lut, idx, 1, 1e-3)
    assert trainer.step_count == 0
    model.close()


# ------------------------------------------------------------------ the command line
def _child(argv, cwd):
    code = ('import json, sys; sys.path.insert(0, %r); import match_main; '
            'from sketchyscenecolorization_amd.matching import MatchConfig; '
            'match_main.main(sys.argv[2:], config=MatchConfig(**json.loads(sys.argv[1])))' % ROOT)
    r = subprocess.run([sys.executable, '-c', code, json.dumps(dict(SMALL, **NARROW))] + argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=CHILD_LIMIT, cwd=cwd)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    return r.stdout.decode()


def _snapshot_bytes(root, n):
    prefix = os.path.join(root, 'deeplab_RMI_iter_%d.tfmodel' % n)
    data = open(prefix + '.data-00000-of-00001', 'rb').read()
    assert len(data) > 0
    return data, open(prefix + '.train_state.json', 'rb').read()


def test_scene_cache_modes_through_the_command_line(split, tmp_path):
    """4 iterations with a snapshot every 2, in fresh processes: the three modes write the same bytes, and so does a run stopped
    at 2 under device and resumed under features."""
    from sketchyscenecolorization_amd import matching as m, tf_checkpoint
    backbone = str(tmp_path / 'backbone-1')
    tf_checkpoint.write_checkpoint(backbone, {k: a for k, a in m.random_variables(split['cfg'], 31).items() if k.startswith('ResNet/')})
    common = ['--mode', 'train', '--backbone_snapshot', backbone, '--vocab_file', VOCAB, '--scene_size', '64', '--save_model_freq', '2',
              '--log_freq', '1', '--seed', '5', '--data_base_dir', split['data'], '--captions_base_dir', os.path.join(split['base'], 'captions')]

    def run(tag, mode, iterations):
        root = str(tmp_path / tag)
        return root, _child(common + ['--snapshot_root', root, '--log_root', root + '_log', '--max_iteration', str(iterations),
                                      '--scene_cache', mode], str(tmp_path))
    roots, printed = {}, {}
    for mode in ('off', 'device', 'features'):
        roots[mode], printed[mode] = run(mode, mode, 4)
    assert 'scene cache:' not in printed['off']
    assert 'scene cache: 2 scenes, 32768 bytes of scenes and 0 of features' in printed['device']
    assert 'scene cache: 2 scenes, 32768 bytes of scenes and 65536 of features' in printed['features']
    for n in (2, 4):
        want = _snapshot_bytes(roots['off'], n)
        for mode in ('device', 'features'):
            assert _snapshot_bytes(roots[mode], n) == want, (mode, n)
    logged = lambda text: [l for l in text.split('\n') if l.startswith('iter = ')]
    assert len(logged(printed['off'])) == 3 and logged(printed['device']) == logged(printed['features']) == logged(printed['off'])
    # stopped at 2 under device, resumed under features
    parts, _ = run('parts', 'device', 2)
    assert _snapshot_bytes(parts, 2) == _snapshot_bytes(roots['off'], 2)
    _, resumed = run('parts', 'features', 4)
    assert 'start_iter 2' in resumed and 'scene cache: 2 scenes' in resumed
    assert _snapshot_bytes(parts, 4) == _snapshot_bytes(roots['off'], 4)
