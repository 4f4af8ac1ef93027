"""The host side of training the matcher's backbone (sketchyscenecolorization_amd/match_backbone_train.py, match_main.py
--train_backbone 1), without a GPU: the oracle tests/match_backbone_oracle.py against
tests/matching_oracle.py, the flags' refusals, the trained and regularised names against a re-enactment of RMI_model.py:320-330,
the snapshot's names, the buffer plan and its budget, and the cases that tests/test_gpu_match_backbone_train.py runs on the device:
their seeds are checked here to give the float32 and the float64 oracle the same sign at every relu and the same argmax in every
pool window."""
import os

import numpy as np
import pytest
import torch

import match_backbone_oracle as BO
import match_eval_oracle as EO
import match_train_oracle as TO
import matching_oracle as MO
from sketchyscenecolorization_amd import match_backbone_train as B, match_train as T, matching as M, tf_checkpoint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = os.path.join(ROOT, 'tests', 'golden', 'match', 'vocab.txt')
# identity units in groups 2, 4 and 5, the stride-2 projection unit in group 3; at rate 4 the sub-images are 2 x 2 at size 64 and
# 3 x 3 at size 96
UNITS, FILTERS = (2, 1, 2, 2), (8, 16, 32, 64, 128)
NARROW = dict(v_emb=24, w_emb=24, w_rnn=40, m_rnn=20)
SEED = 11
DESCENT = dict(steps=30, lr=1e-3, weight_decay=5e-4)


def small_config(size=64):
    return M.MatchConfig(size=size, units=UNITS, filters=FILTERS, **NARROW)


def gradient_case(size, seed=SEED, fresh_head=False):
    """One (scene, caption) of the small model -> (config, variables, sketch, labels, indices, seq_len, the target's label)."""
    cfg = small_config(size)
    v = M.random_variables(cfg, seed)
    if fresh_head:
        v.update(T.init_head(cfg, seed))
    rng = np.random.RandomState(seed + 1)
    sk = np.full((size, size, 3), 255, np.uint8)
    sk[rng.rand(size, size) < 0.5] = 0
    labels = np.zeros((size, size), np.uint8)
    labels[4:30, 6:40], labels[34:60, 20:62] = 1, 2
    idx = np.random.RandomState(seed + 2).randint(2, cfg.vocab_size, cfg.max_len)
    idx[5:] = 0
    return cfg, v, sk, labels, idx.astype(np.int64), 5, 2


_ORACLE = {}


def oracle_gradients(size):
    """The float64 and the float32 oracle on ``gradient_case(size)``, computed once for the session and left unchanged:
    {dtype: (loss, gradients, pred, feat, record)}."""
    if size not in _ORACLE:
        cfg, v, sk, labels, idx, L, label = gradient_case(size)
        _ORACLE[size] = {dt: BO.loss_and_gradients(sk, v, idx, L, labels == label, UNITS, FILTERS, dt)
                         for dt in (torch.float64, torch.float32)}
    return _ORACLE[size]


_DESCENT = {}


def oracle_descent(train_backbone):
    """The class losses of DESCENT['steps'] iterations of the oracle on gradient_case(64) with a fresh head -> {dtype: losses}."""
    if train_backbone not in _DESCENT:
        cfg, v, sk, labels, idx, L, label = gradient_case(64, fresh_head=True)
        _DESCENT[train_backbone] = {dt: BO.train(sk, v, idx, L, labels == label, UNITS, FILTERS, DESCENT['steps'], DESCENT['lr'],
                                                 DESCENT['weight_decay'], train_backbone, dt)[0]
                                    for dt in (torch.float64, torch.float32)}
    return _DESCENT[train_backbone]


# ------------------------------------------------------------------ the oracle itself
@pytest.mark.parametrize('size', [64, 96])
def test_oracle_forward_equals_the_matching_oracle(size):
    cfg, v, sk, labels, idx, L, label = gradient_case(size)
    _up, _predicts, want = MO.forward(sk, v, idx.tolist(), L, UNITS, FILTERS, cfg.max_len)
    loss, grads, pred, feat, _rec = oracle_gradients(size)[torch.float64]
    assert pred.shape == want.shape == (size // 8, size // 8) and np.abs(want).max() > 0
    assert np.abs(pred - want).max() <= 1e-12 * np.abs(want).max()
    x, _stroke = MO.preprocess(sk)
    assert np.abs(feat - MO.backbone(x[None], {k: np.asarray(a, np.float64) for k, a in v.items()}, UNITS, FILTERS)).max() <= 1e-12 * feat.max()
    assert set(grads) == set(BO.trained_names(v)) and all(g.any() and np.isfinite(g).all() for g in grads.values())
    assert loss > 0


@pytest.mark.parametrize('size', [64, 96])
def test_the_cases_of_the_device_tests_flip_no_mask_between_float32_and_float64(size):
    o = oracle_gradients(size)
    ok, what = BO.records_agree(o[torch.float32][4], o[torch.float64][4])
    assert ok, what
    kinds = [w for w, _ in o[torch.float64][4]]
    assert kinds[:2] == ['conv1', 'pool argmax'] and len(kinds) == 2 + 3 * sum(UNITS)
    # every relu is live on both sides: a mask of all ones or all zeros would test nothing
    assert all(0 < a.mean() < 1 for w, a in o[torch.float64][4] if w != 'pool argmax')


def test_the_oracle_shows_a_clear_gap_between_training_the_backbone_and_not():
    both, head = oracle_descent(True)[torch.float64], oracle_descent(False)[torch.float64]
    print('float64 oracle, %d steps: backbone %.6g -> %.6g, head alone %.6g -> %.6g' % (DESCENT['steps'], both[0], both[-1], head[0], head[-1]))
    assert both[0] == head[0] and head[-1] < 0.75 * head[0] and both[-1] < 0.85 * head[-1]


# ------------------------------------------------------------------ names
def test_trained_and_regularised_names_are_the_references():
    cfg = M.MatchConfig()
    shapes = cfg.variable_shapes()
    trainable = [(n, n.rsplit('/', 1)[1] not in M.NORM_PARTS) for n in shapes]
    for fusion_only in (False, True):
        tvars, reg = BO.reference_trained_and_regularized(trainable, fusion_only)
        assert B.trained_variable_names(cfg, not fusion_only) == tvars
        assert [n for n in B.trained_variable_names(cfg, not fusion_only) if T.is_regularized(n)] == reg
    names = B.backbone_variable_names(cfg)
    assert len(names) == 1 + 3 * 33 + 4 == 104 and len(B.trained_variable_names(cfg, True)) == 104 + 9
    assert len([n for n in B.trained_variable_names(cfg, True) if T.is_regularized(n)]) == 106
    assert all(T.grad_scale(n) == 1.0 for n in names)          # no backbone variable is a 'biases'


def test_snapshot_names_and_the_slotless_refusal():
    cfg = small_config()
    v = M.random_variables(cfg, 3)
    model = M.MatchModel(cfg, device='cpu')
    model.load_dict(v)
    trainer = B.BackboneMatchTrainer(model)
    names = B.backbone_variable_names(cfg)
    assert len(names) == 1 + 3 * sum(UNITS) + 4
    # the spans are the filters, and nothing of a norm table is inside one
    lay = model._layout
    for n in names:
        o, size, padded, shape = trainer.b_spans[n]
        assert (o, shape) == lay[n] and size == int(np.prod(shape)) and padded == -(-size // 64) * 64
    tensors = trainer.snapshot_tensors()
    head = T.head_variable_names(cfg)
    want = set(cfg.variable_shapes()) | {n + s for n in names + head for s in ('/Adam', '/Adam_1')} | {'beta1_power', 'beta2_power', 'Variable'}
    assert set(tensors) == want
    for n in names:
        assert tensors[n + '/Adam'].shape == tensors[n + '/Adam_1'].shape == tuple(cfg.variable_shapes()[n])
        assert np.array_equal(tensors[n], v[n])
    fresh = M.MatchModel(cfg, device='cpu')
    fresh.load_dict(tensors)            # --mode match and --mode eval read it as it is
    assert torch.equal(fresh.flat, model.flat)
    trainer.load_slots(tensors, 0)
    # a snapshot of the head's trainer has no slots of the backbone: each trainer says so, the head's ignores the extras
    plain = T.MatchTrainer(fresh).snapshot_tensors()
    with pytest.raises(ValueError, match=r'ResNet/group_1/conv1/DW/Adam.*--train_backbone 0'):
        trainer.load_slots(plain, 2)
    T.MatchTrainer(fresh).load_slots(tensors, 2)
    model.close()
    fresh.close()


# ------------------------------------------------------------------ the buffer plan
def test_buffer_plan_and_budget():
    cfg = small_config()
    geo = B.unit_geometry(cfg)
    assert [g[4] for g in geo] == [0, 0, 0, 1, 0, 1, 0] and geo[2][3] == 2
    assert geo[2][5] == (1, 16, 16, 16) and geo[2][6] == (1, 8, 8, 32) and geo[-1][6] == (16, 2, 2, 128)
    fwd = B.forward_buffer_shapes(cfg)
    assert fwd['bt/s2b2'] == (4, 4, 4, 32) and fwd['bt/s2b4'] == (16, 2, 2, 64) and fwd['bt/b2s2'] == (4, 4, 4, 128) and fwd['bt/b2s1'] == (1, 8, 8, 128)
    assert 'bt/ResNet/group_3_0/sc' in fwd and 'bt/ResNet/group_2_1/sc' not in fwd
    act, scratch, slots = B.training_bytes(M.MatchConfig())
    print('released size: %d bytes of activations, %d of scratch, %d of gradient and slots' % (act, scratch, slots))
    assert 3.0e9 < act < 4.5e9 and 0.4e9 < slots < 0.6e9
    with pytest.raises(ValueError, match=str(act)):
        B.check_budget(M.MatchConfig(), 2 * (act + scratch + slots) - 2)
    assert B.check_budget(M.MatchConfig(), 2 * (act + scratch + slots)) == (act, scratch, slots)


# ------------------------------------------------------------------ the flags
def test_train_backbone_flag_is_checked_before_anything_is_read(tmp_path):
    import match_main
    cfg = M.MatchConfig(size=64, units=(1, 1, 1, 1), filters=FILTERS)
    backbone = str(tmp_path / 'backbone-1')
    tf_checkpoint.write_checkpoint(backbone, {k: a for k, a in M.random_variables(cfg, 0).items() if k.startswith('ResNet/')})
    flags = EO.write_split(str(tmp_path), 'train')[:4]
    snaps, logs = str(tmp_path / 'snapshots'), str(tmp_path / 'log')
    good = ['--mode', 'train', '--backbone_snapshot', backbone, '--vocab_file', VOCAB, '--scene_size', '64', '--snapshot_root', snaps,
            '--log_root', logs, '--max_iteration', '4'] + flags
    assert match_main.build_parser().parse_args([]).train_backbone == 0
    for extra in (['--train_backbone', '1'], ['--train_backbone', '1', '--scene_cache', 'device'], ['--train_backbone', '1', '--scene_cache', 'off'],
                  ['--train_backbone', '0', '--scene_cache', 'features']):
        match_main.checked_train_arguments(match_main.build_parser().parse_args(good + extra))
    for extra, match in ((['--train_backbone', '2'], 'train_backbone 2'), (['--train_backbone', '-1'], 'train_backbone'),
                         (['--train_backbone', '1', '--scene_cache', 'features'], '--scene_cache device'),
                         (['--train_fusion_var_only', '0'], r'train_fusion_var_only.*--train_backbone')):
        with pytest.raises(ValueError, match=match):
            match_main.main(good + extra)
        assert not os.path.exists(snaps) and not os.path.exists(logs)
