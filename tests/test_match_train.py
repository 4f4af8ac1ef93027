"""The host side of training the matcher's fusion head (sketchyscenecolorization_amd/match_train.py, match_main.py --mode train),
without a GPU: the layout round trip, the schedule, the order of the tuples, the name rules, the flags' refusals, and the oracle
tests/match_train_oracle.py against tests/matching_oracle.py."""
import json
import os
import random
import sys

import numpy as np
import pytest
import torch

import match_eval_oracle as EO
import match_train_oracle as TO
import matching_oracle as MO
from sketchyscenecolorization_amd import match_eval, match_train as T, matching as M, tf_checkpoint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = os.path.join(ROOT, 'tests', 'golden', 'match', 'vocab.txt')
SMALL = dict(size=64, units=(1, 1, 1, 1), filters=(8, 16, 32, 64, 128))


# ------------------------------------------------------------------ the layout round trip
@pytest.mark.parametrize('widths', [dict(v_emb=24, w_emb=24, w_rnn=40, m_rnn=20), dict(v_emb=1000, w_emb=1000, w_rnn=1000, m_rnn=500)])
def test_export_inverts_load_bit_for_bit(widths):
    cfg = M.MatchConfig(**dict(SMALL, **widths))
    assert (M.pad32(cfg.w_rnn), M.pad32(cfg.m_rnn)) in ((64, 32), (1024, 512))
    v = M.random_variables(cfg, 3)
    model = M.MatchModel(cfg, device='cpu')
    model.load_dict(v)
    flat = model.flat.clone()
    trainer = T.MatchTrainer(model)
    out = trainer.export_variables()
    assert set(out) == set(v) == set(cfg.variable_shapes())
    for name, a in v.items():
        assert out[name].dtype == np.float32 and out[name].shape == a.shape and np.array_equal(out[name], a), name
    model.flat.zero_()
    model.load_dict(out)
    assert torch.equal(model.flat, flat)
    # pack_head is load_dict's layout, unpack_head its inverse
    dev = T.pack_head(cfg, v)
    for name in T.HEAD_DEVICE_NAMES:
        assert np.array_equal(dev[name].reshape(-1), model.d[name].numpy().reshape(-1)), name
    back = T.unpack_head(cfg, dev)
    assert all(np.array_equal(back[n], v[n]) for n in T.head_variable_names(cfg))
    # the head is one stretch of the flat buffer and spatial is not in it
    assert trainer.hi == model._layout['spatial'][0] and trainer.params.numel() == trainer.grad.numel() == trainer.hi - trainer.lo
    assert sum(p for _o, _s, p, _sh in trainer.spans.values()) == trainer.hi - trainer.lo
    model.close()


def test_initial_variables_have_the_parents_bits():
    """profiles/match_forward_once.txt keeps the digests scripts/match_forward_digest.py printed on the parent commit's tree; its
    ``host`` lines are random_variables(cfg, 41) and init_head(cfg, 5) of both head widths with the attention off and on, which
    every recorded digest and parity file rests on.  This tree's are the same."""
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    try:
        import match_forward_digest as D
    finally:
        sys.path.pop(0)
    want = {k: v for k, v in D.recorded(os.path.join(ROOT, 'profiles', 'match_forward_once.txt')).items() if ' host ' in k}
    got = dict(line for case in D.CASES for line in D.host_digests(*case))
    assert len(want) == 8 and set(got) == set(want), set(got) ^ set(want)
    for what, sha in got.items():
        assert sha == want[what], what


def test_init_head_follows_the_reference_initialisers():
    cfg = M.MatchConfig(**dict(SMALL, v_emb=24, w_emb=24, w_rnn=40, m_rnn=20))
    a, b = T.init_head(cfg, 5), T.init_head(cfg, 5)
    assert set(a) == set(T.head_variable_names(cfg)) and all(np.array_equal(a[k], b[k]) for k in a)
    assert not np.array_equal(a[TO.P + 'embedding'], T.init_head(cfg, 6)[TO.P + 'embedding'])
    shapes = cfg.variable_shapes()
    for name, v in a.items():
        assert v.dtype == np.float32 and v.shape == tuple(shapes[name])
        leaf = name.rsplit('/', 1)[1]
        if leaf in ('bias', 'biases'):
            assert not v.any()
        elif leaf == 'embedding':
            assert 0.07 < np.abs(v).max() <= 0.08
        else:
            fan = (shapes[name][2] + shapes[name][3]) if leaf == 'DW' else (shapes[name][0] + shapes[name][1])
            lim = np.sqrt(6.0 / fan)
            assert 0.9 * lim < np.abs(v).max() <= lim * (1 + 1e-6)


# ------------------------------------------------------------------ the schedule
def test_polynomial_decay():
    want = {0: 2.5e-4, 1: (2.5e-4 - 1e-5) * (1 - 1 / 75000) ** 0.9 + 1e-5, 74999: (2.5e-4 - 1e-5) * (1 / 75000) ** 0.9 + 1e-5, 75000: 1e-5,
            10 ** 5: 1e-5}
    for step, lr in want.items():
        assert T.polynomial_decay(step) == pytest.approx(lr, rel=1e-12), step
        assert T.polynomial_decay(step) == pytest.approx(TO.polynomial_decay(step), rel=1e-12)
    assert T.polynomial_decay(0) > T.polynomial_decay(1) > T.polynomial_decay(74999) > T.polynomial_decay(75000)
    assert T.polynomial_decay(5, 1e-3, 1e-4, 10) == pytest.approx((1e-3 - 1e-4) * 0.5 ** 0.9 + 1e-4, rel=1e-12)
    assert T.adam_step_size(0.5, 1) == pytest.approx(0.5 * np.sqrt(1 - 0.999) / (1 - 0.9), rel=1e-12)


# ------------------------------------------------------------------ the name rules
def test_bias_doubling_and_regulariser_follow_the_canonical_names():
    cfg = M.MatchConfig(**SMALL)
    names = T.head_variable_names(cfg)
    assert names == TO.HEAD_NAMES
    assert [n[len(TO.P):] for n in names if T.grad_scale(n) == 2.0] == ['visual_feat_projection/biases', 'm_lstm_output_projection/biases']
    assert all(T.grad_scale(n) == 1.0 for n in names if 'lstm_cell' in n or n.endswith('embedding') or n.endswith('DW'))
    assert [n[len(TO.P):] for n in names if T.is_regularized(n)] == ['visual_feat_projection/DW', 'm_lstm_output_projection/DW']
    assert set(T.DEVICE_TO_VARIABLE.values()) == set(n[len(TO.P):] for n in names)
    assert [d for d, n in T.DEVICE_TO_VARIABLE.items() if T.grad_scale(n) == 2.0] == ['vproj/b', 'proj/b']
    assert [d for d, n in T.DEVICE_TO_VARIABLE.items() if T.is_regularized(n)] == ['vproj/w', 'proj/w']


# ------------------------------------------------------------------ the order of the tuples
@pytest.mark.parametrize('seed', [0, 7])
def test_order_and_captions_equal_the_reference_loop(tmp_path, seed):
    EO.write_split(str(tmp_path), 'train')
    tuples = T.training_tuples(match_eval.read_captions(str(tmp_path / 'captions'), 'train'))
    assert len(tuples) == 6 and tuples[1] == ('11', 'two trees on the right', [1, 3])
    want = TO.reference_order(tuples, seed, 20, match_eval.augment_caption)
    cursor = T.TupleCursor(len(tuples), random.Random(seed))
    got = []
    for n in range(20):
        if n == 8:          # a snapshot in between: the saved state, through JSON, continues the same sequence
            state = json.loads(json.dumps(cursor.state()))
            cursor = T.TupleCursor(len(tuples), random.Random(12345))
            cursor.restore(state)
        k = cursor.next()
        got.append((k, match_eval.augment_caption(tuples[k][1], cursor.rng)))
    assert got == want
    assert sorted(k for k, _ in got[:6]) == sorted(k for k, _ in got[6:12]) == list(range(6))
    assert [k for k, _ in got[:6]] != [k for k, _ in got[6:12]]
    with pytest.raises(ValueError):
        T.TupleCursor(5, random.Random(0)).restore(state)
    with pytest.raises(ValueError):
        T.TupleCursor(0, random.Random(0))


def test_caption_lut_and_snapshot_names():
    lut = T.caption_lut([3, 5, 3])
    assert lut.dtype == np.uint8 and lut.shape == (256,) and lut.nonzero()[0].tolist() == [3, 5]
    p = T.snapshot_prefix('some/root', 30000)
    assert p == os.path.join('some/root', 'deeplab_RMI_iter_30000.tfmodel') and T.snapshot_iteration(p) == 30000
    with pytest.raises(ValueError):
        T.snapshot_iteration('some/root/model-3')


# ------------------------------------------------------------------ the flags
def test_train_mode_checks_its_arguments_before_anything_is_read(tmp_path):
    import match_main
    cfg = M.MatchConfig(**SMALL)
    backbone = str(tmp_path / 'backbone-1')
    tf_checkpoint.write_checkpoint(backbone, {k: v for k, v in M.random_variables(cfg, 0).items() if k.startswith('ResNet/')})
    flags = EO.write_split(str(tmp_path), 'train')[:4]          # --data_base_dir, --captions_base_dir
    snaps, logs = str(tmp_path / 'snapshots'), str(tmp_path / 'log')
    good = ['--mode', 'train', '--backbone_snapshot', backbone, '--vocab_file', VOCAB, '--scene_size', '64', '--vocab_size', '76',
            '--text_len', '15', '--snapshot_root', snaps, '--log_root', logs, '--max_iteration', '4', '--save_model_freq', '2',
            '--log_freq', '1', '--seed', '3', '--start_lr', '2.5e-4', '--end_lr', '1e-5', '--lr_decay_step', '75000',
            '--weight_decay', '5e-4'] + flags
    cfg2, vocab, tuples, resume, bb = match_main.checked_train_arguments(match_main.build_parser().parse_args(good))
    assert (cfg2.size, len(vocab), len(tuples), resume, bb) == (64, 76, 6, None, backbone)
    d = match_main.build_parser().parse_args([])
    assert (d.backbone_snapshot, d.snapshot_root, d.max_iteration, d.save_model_freq, d.log_freq, d.seed, d.start_lr, d.end_lr,
            d.lr_decay_step, d.weight_decay, d.log_root) == ('', 'outputs/snapshots', 100000, 10000, 50, 0, 2.5e-4, 1e-5, 75000, 5e-4,
                                                             'outputs/log')

    def bad(extra=(), match=None, **change):
        argv = list(good) + list(extra)
        for k, val in change.items():
            i = argv.index('--' + k)
            if val is None:
                del argv[i:i + 2]
            else:
                argv[i + 1] = val
        with pytest.raises(ValueError, match=match):
            match_main.main(argv)
        assert not os.path.exists(snaps) and not os.path.exists(logs)
    bad(backbone_snapshot=None, match='backbone_snapshot')
    bad(backbone_snapshot=str(tmp_path / 'nothing'))
    bad(max_iteration='0')
    bad(save_model_freq='0')
    bad(log_freq='0')
    bad(start_lr='0')
    bad(end_lr='-1')
    bad(lr_decay_step='0')
    bad(weight_decay='-1')
    bad(snapshot_root='')
    bad(log_root='')
    bad(scene_size='72')
    bad(text_len='0')
    bad(vocab_size='75')
    bad(vocab_file=str(tmp_path / 'no_vocab.txt'))
    bad(data_base_dir=str(tmp_path / 'no_data'))
    bad(captions_base_dir=str(tmp_path / 'no_captions'))
    for flag, val in (('train_fusion_var_only', '0'), ('training_ignore_bg', '0'), ('batch_size', '2'), ('gpus', '2'), ('graph', '1'),
                      ('keep_prob', '0.5'), ('weights', 'fcn_8s'), ('fusion_type', 'RecurAttn'), ('summary', '1')):
        bad(extra=['--' + flag, val], match=flag)
    # a vocabulary whose row 0 is not <pad>
    words = open(VOCAB).read().split('\n')
    assert words[0] == '<pad>'
    words[0], words[2] = words[2], words[0]
    other = tmp_path / 'vocab_pad_elsewhere.txt'
    other.write_text('\n'.join(words))
    bad(vocab_file=str(other), match='<pad>')
    # a caption without a category, and a missing file of the LAST scene
    path = str(tmp_path / 'captions' / 'sentence_instance_train.json')
    data = json.load(open(path))
    data[1]['sen_instIdx_map']['the thing on the left'] = [0]
    json.dump(data, open(path, 'w'))
    bad(match='category')
    del data[1]['sen_instIdx_map']['the thing on the left']
    json.dump(data, open(path, 'w'))
    match_main.checked_train_arguments(match_main.build_parser().parse_args(good))
    os.remove(str(tmp_path / 'data' / 'train' / 'DRAWING_GT' / 'L0_sample12.png'))
    bad(match='L0_sample12')
    # a snapshot root with a checkpoint but no training state cannot be resumed from
    os.makedirs(snaps)
    tf_checkpoint.write_checkpoint(T.snapshot_prefix(snaps, 2), M.random_variables(cfg, 0))
    with open(os.path.join(snaps, 'checkpoint'), 'w') as f:
        f.write('model_checkpoint_path: "deeplab_RMI_iter_2.tfmodel"\n')
    with pytest.raises(ValueError, match='train_state'):
        match_main.main(good)


# ------------------------------------------------------------------ the oracle itself
def _case(seed, widths, feat_hw=4, F=16, seq_len=3, T_len=15, vocab=76):
    rng = np.random.RandomState(seed)
    cfg = M.MatchConfig(size=8 * feat_hw if feat_hw % 4 == 0 else 32, units=(1, 1, 1, 1), filters=(8, 16, 32, 64, F), vocab_size=vocab,
                        max_len=T_len, **widths)
    v = {k: a for k, a in M.random_variables(cfg, seed).items() if k.startswith(TO.P)}
    feat = np.maximum(rng.randn(1, feat_hw, feat_hw, F), 0)
    idx = rng.randint(2, vocab, T_len)
    idx[seq_len:] = 0
    return v, feat, idx.tolist()


def test_oracle_head_equals_the_matching_oracle():
    v, feat, idx = _case(1, dict(v_emb=24, w_emb=24, w_rnn=40, m_rnn=20))
    want = MO.head(feat, {k: a.astype(np.float64) for k, a in v.items()}, idx, 3, 15)
    t = {k: torch.tensor(a, dtype=torch.float64) for k, a in v.items()}
    got = TO.head(torch.tensor(feat, dtype=torch.float64), t, idx, 3).numpy()
    assert np.abs(want).max() > 1e-3 and np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_oracle_resize_matrix_equals_the_legacy_resize():
    rng = np.random.RandomState(2)
    for h, S in ((4, 32), (12, 96), (5, 20)):
        pred = rng.randn(h, h)
        A = TO.resize_matrix(h, S)
        assert np.allclose(A.sum(axis=1), 1) and (A[-S // h:, :-1] == 0).all() and (A[-S // h:, -1] == 1).all()      # the clamp band
        assert np.abs(A @ pred @ A.T - MO.resize_bilinear_legacy(pred, S)).max() <= 1e-13


def test_oracle_closed_form_dpred_equals_autograd():
    rng = np.random.RandomState(3)
    for h, S in ((4, 32), (8, 64)):
        pred = rng.randn(h, h) * 2
        sk = rng.choice(np.array([0, 50, 104, 105, 254, 255], np.uint8), (S, S, 3))
        target = rng.rand(S, S) < 0.4
        loss, live, grad = TO.loss_on_pred(pred, sk, target)
        assert live == int((sk[:, :, 0] <= 104).sum()) and 0 < live < S * S
        up = MO.resize_bilinear_legacy(pred, S)
        per = np.maximum(up, 0) - up * target + np.log1p(np.exp(-np.abs(up)))
        assert loss == pytest.approx(float(per[sk[:, :, 0] <= 104].sum()), rel=1e-12)
        want = TO.dpred_closed_form(pred, sk, target)
        assert np.abs(grad - want).max() <= 1e-12 * np.abs(want).max()


def test_oracle_adam_is_tf_adam():
    var, g = np.array([1.0, -2.0]), np.array([0.5, -0.25])
    w1, m1, v1 = TO.adam_tf(var, g, np.zeros(2), np.zeros(2), 0.1, 1)
    assert np.allclose(m1, 0.1 * g) and np.allclose(v1, 0.001 * g * g)
    lr_t = 0.1 * np.sqrt(1 - 0.999) / (1 - 0.9)
    assert np.allclose(w1, var - lr_t * m1 / (np.sqrt(v1) + 1e-8), rtol=1e-15)
    w, _m, _v = TO.update(TO.P + 'visual_feat_projection/biases', var, g, np.zeros(2), np.zeros(2), 0.1, 1)
    assert np.allclose(w, TO.adam_tf(var, 2 * g, np.zeros(2), np.zeros(2), 0.1, 1)[0], rtol=1e-15)
    w, _m, _v = TO.update(TO.P + 'visual_feat_projection/DW', var, g, np.zeros(2), np.zeros(2), 0.1, 1, 0.5)
    assert np.allclose(w, TO.adam_tf(var, g + 0.5 * var, np.zeros(2), np.zeros(2), 0.1, 1)[0], rtol=1e-15)
    w, _m, _v = TO.update(TO.P + 'wLSTM/lstm_cell/bias', var, g, np.zeros(2), np.zeros(2), 0.1, 1)
    assert np.allclose(w, w1, rtol=1e-15)


# ------------------------------------------------------------------ the learning case of tests/test_gpu_match_train.py
LEARN = dict(seed=41, lr=1e-2, steps=40)


def learning_case():
    """One (scene, caption) of the small model with a fresh head -> (config, variables, scene, lut, indices, seq_len)."""
    cfg = M.MatchConfig(**dict(SMALL, v_emb=24, w_emb=24, w_rnn=40, m_rnn=20))
    v = M.random_variables(cfg, LEARN['seed'])
    v.update(T.init_head(cfg, LEARN['seed']))
    rng = np.random.RandomState(1)
    sk = np.full((64, 64, 3), 255, np.uint8)
    sk[rng.rand(64, 64) < 0.5] = 0
    labels = np.zeros((64, 64), np.uint8)
    labels[4:30, 6:40], labels[34:60, 20:62] = 1, 2
    idx = np.random.RandomState(2).randint(2, cfg.vocab_size, cfg.max_len)
    idx[5:] = 0
    return cfg, v, {'sketch': sk, 'labels': labels}, T.caption_lut([2]), idx.astype(np.int64), 5


def test_the_learning_case_learns_in_float64():
    """40 steps of the float64 oracle on the learning case: the class loss falls below a quarter of the first, which leaves the
    device's test (below half) room to spare."""
    cfg, v, scene, lut, idx, L = learning_case()
    v64 = {k: a.astype(np.float64) for k, a in v.items()}
    x, _stroke = MO.preprocess(scene['sketch'])
    feat = MO.backbone(x[None], v64, cfg.units, cfg.filters)
    target = lut[scene['labels']] != 0
    head = {k: v64[k] for k in TO.HEAD_NAMES}
    slots = {k: (np.zeros_like(a), np.zeros_like(a)) for k, a in head.items()}
    losses = []
    for t in range(1, LEARN['steps'] + 1):
        loss, grads, _pred = TO.train_step_loss(feat, head, idx, L, scene['sketch'], target)
        losses.append(loss)
        for k in head:
            head[k], m, s = TO.update(k, head[k], grads[k], slots[k][0], slots[k][1], LEARN['lr'], t)
            slots[k] = (m, s)
    print('float64 oracle: first %.6g, last %.6g' % (losses[0], losses[-1]))
    assert losses[-1] < 0.25 * losses[0]
