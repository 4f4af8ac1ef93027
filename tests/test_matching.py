"""The host side of the instance matcher (sketchyscenecolorization_amd/matching.py, match_main.py), without a GPU: text processing,
the spatial table and the selection against what the reference's functions returned (tests/golden/match/, recorded by
tests/golden/make_match_goldens.py), the norm folding and the LSTM padding against their formulas, the checkpoint names, the
space-to-batch argument against a direct dilated conv, and the command line's refusals."""
import json
import os

import numpy as np
import pytest

import matching_oracle as O
from sketchyscenecolorization_amd import matching as M
from sketchyscenecolorization_amd import tf_checkpoint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'match')
SMALL = dict(size=64, units=(2, 1, 2, 2), filters=(8, 16, 32, 64, 128), v_emb=24, w_emb=16, w_rnn=20, m_rnn=12)


def _vocab():
    return M.load_vocab(os.path.join(GOLD, 'vocab.txt'))


# ------------------------------------------------------------------ goldens
def test_vocab_is_the_matchers_76_words():
    v = _vocab()
    assert len(v) == 76 and v['<pad>'] == 0 and v['<unk>'] == 1


def test_sentences_equal_the_reference():
    v = _vocab()
    cases = json.load(open(os.path.join(GOLD, 'text.json')))
    assert len(cases) >= 20
    assert any(c['seq_len'] == 15 and len(M.sentence_tokens(c['sentence'])) > 15 for c in cases)        # a cut one
    assert any(c['sentence'].rstrip().endswith('.') for c in cases) and any('-' in c['sentence'] for c in cases)
    assert any(v['<unk>'] in c['indices'][:c['seq_len']] for c in cases)
    for c in cases:
        assert M.preprocess_sentence(c['sentence'], v, 15) == (c['indices'], c['seq_len']), c['sentence']
        assert O.sentence(c['sentence'], v, 15) == (c['indices'], c['seq_len']), c['sentence']
        assert c['indices'][c['seq_len']:] == [v['<pad>']] * (15 - c['seq_len'])       # padded on the right


@pytest.mark.parametrize('text', ['', '   ', '.', ' - ', ' . '])
def test_a_sentence_without_a_token_is_refused(text):
    with pytest.raises(ValueError):
        M.preprocess_sentence(text, _vocab(), 15)


def test_spatial_table_equals_the_reference():
    with np.load(os.path.join(GOLD, 'spatial.npz')) as z:
        for key in ('8x8', '12x12'):
            h, w = (int(s) for s in key.split('x'))
            assert M.spatial_features(h, w).dtype == np.float32
            assert np.array_equal(M.spatial_features(h, w), z[key]), key
            assert np.array_equal(O.spatial(h, w), z[key]), key


def _selection(size):
    with np.load(os.path.join(GOLD, 'selection.npz')) as z:
        tag = 's%d/' % size
        n = int(z[tag + 'n'])
        return (z[tag + 'predicts'], z[tag + 'boxes'], [z[tag + 'mask_%d' % k] for k in range(n)], z[tag + 'matched'].tolist(),
                z[tag + 'scores'])


@pytest.mark.parametrize('size', [64, 96])
def test_selection_equals_the_reference(size):
    predicts, boxes, masks, matched, scores = _selection(size)
    counts = O.occupancy(predicts, boxes, masks)
    got, got_scores = M.select_instances(counts)
    assert got == matched == O.select(counts)[0]
    assert np.array_equal(got_scores, scores, equal_nan=True)           # float64 equality
    k = [i for i, s in enumerate(scores) if s == 0.5]
    assert k and not set(k) & set(matched)                              # exactly one half: not matched
    empty = [i for i, m in enumerate(masks) if not m.any()]
    assert empty and all(np.isnan(scores[i]) for i in empty) and not set(empty) & set(matched)
    big = [i for i, m in enumerate(masks) if m.max() > 1]               # bytes summed below, pixels counted above
    assert big and any(counts[i, 1] > np.count_nonzero(masks[i]) for i in big)


def test_pack_masks_refuses_bad_boxes():
    m = np.ones((3, 4), np.uint8)
    buf, off = M.pack_masks([[1, 2, 3, 5], [0, 0, 2, 3]], [m, m], 8)
    assert buf.shape == (24,) and off.tolist() == [0, 12]
    for box, mask in (([1, 2, 3, 8], m), ([-1, 2, 1, 5], m), ([1, 2, 3, 5], np.ones((3, 3), np.uint8)), ([3, 2, 2, 5], np.ones((0, 4), np.uint8))):
        with pytest.raises(ValueError):
            M.pack_masks([box], [mask], 8)


# ------------------------------------------------------------------ folding and padding
def test_norm_folding_is_the_formula():
    rng = np.random.RandomState(0)
    c = 12
    beta, gamma, mean = rng.randn(c), rng.uniform(0.5, 2, c), rng.randn(c)
    var, factor = rng.uniform(0.1, 3, c), np.array([1.7])
    ab = M.fold_norm(beta, gamma, factor, mean, var)
    assert ab.dtype == np.float32 and ab.shape == (2 * c,)
    x = rng.randn(5, c)
    want = (x - mean / factor) / np.sqrt(var / factor + 0.001) * gamma + beta
    got = x * ab[:c].astype(np.float64) + ab[c:].astype(np.float64)
    assert np.abs(got - want).max() <= 2.0 ** -23 * (np.abs(x).max() * np.abs(ab[:c]).max() + np.abs(ab[c:]).max())
    v = {'s/beta': beta, 's/gamma': gamma, 's/factor': factor, 's/mean': mean, 's/variance': var}
    assert np.allclose(O.norm(x, v, 's'), want, rtol=0, atol=1e-12)


def _cell(x, c, h, kx, kh, b):
    z = x @ kx + h @ kh + b
    i, j, f, o = np.split(z, 4, axis=1)
    c1 = c * O.sigmoid(f + 1) + O.sigmoid(i) * np.tanh(j)
    return c1, np.tanh(c1) * O.sigmoid(o)


def test_gate_block_padding_changes_no_real_value():
    rng = np.random.RandomState(1)
    n_in, c = 7, 20
    kernel, bias = rng.randn(n_in + c, 4 * c) * 0.3, rng.randn(4 * c) * 0.3
    kx, kh, b = M.pad_lstm(kernel, bias, n_in, c)
    cp = M.pad32(c)
    assert cp == 32 and kx.shape == (n_in, 4 * cp) and kh.shape == (cp, 4 * cp) and b.shape == (4 * cp,)
    cs, hs = np.zeros((3, c)), np.zeros((3, c))
    cpd, hpd = np.zeros((3, cp)), np.zeros((3, cp))
    for t in range(5):
        x = rng.randn(3, n_in)
        cs, hs = O.lstm_cell(x, cs, hs, kernel, bias)
        cpd, hpd = _cell(x, cpd, hpd, kx, kh, b)
        assert np.array_equal(cpd[:, c:], np.zeros((3, cp - c))) and np.array_equal(hpd[:, c:], np.zeros((3, cp - c)))
        assert np.allclose(cpd[:, :c], cs, rtol=0, atol=1e-14) and np.allclose(hpd[:, :c], hs, rtol=0, atol=1e-14)
    assert M.pad32(1000) == 1024 and M.pad32(500) == 512 and M.pad32(512) == 512


# ------------------------------------------------------------------ configuration and checkpoint names
def test_config_refusals():
    M.MatchConfig(**SMALL)
    for bad in (dict(size=72), dict(size=0), dict(filters=(8, 16, 32, 64, 120)), dict(filters=(6, 16, 32, 64, 128)), dict(m_rnn=10),
                dict(units=(2, 1, 2)), dict(units=(2, 0, 2, 2))):
        with pytest.raises(ValueError):
            M.MatchConfig(**dict(SMALL, **bad))
    cfg = M.MatchConfig()
    assert (cfg.size, cfg.units, cfg.filters, cfg.vocab_size, cfg.max_len) == (768, (3, 4, 23, 3), (64, 256, 512, 1024, 2048), 76, 15)
    shapes = cfg.variable_shapes()
    assert shapes['ResNet/group_1/conv1/DW'] == (7, 7, 3, 64) and shapes['ResNet/group_1/bn_conv1/factor'] == (1,)
    assert shapes['ResNet/group_4_0/block_add/conv/DW'] == (1, 1, 512, 1024) and 'ResNet/group_4_1/block_add/conv/DW' not in shapes
    assert shapes['ResNet/group_4_22/block_2/conv/DW'] == (3, 3, 256, 256) and 'ResNet/group_4_23/block_1/conv/DW' not in shapes
    assert shapes['text_sketchyscene/mLSTM/lstm_cell/kernel'] == (3508, 2000)
    assert shapes['text_sketchyscene/wLSTM/lstm_cell/kernel'] == (2000, 4000)
    units = cfg.net.unit_list()
    assert [u for u in units if u[3] == 2] == [('ResNet/group_3_0', 256, 512, 2, 1)]
    assert {u[4] for u in units if u[0].startswith('ResNet/group_4')} == {2} and {u[4] for u in units if u[0].startswith('ResNet/group_5')} == {4}


class _Host(M.MatchModel):
    """load_dict's checks and layouts without a device: the flat buffer on the CPU."""

    def __init__(self, config):
        import torch
        self.cfg, self.device = config, torch.device('cpu')
        self.cw, self.cm = M.pad32(config.w_rnn), M.pad32(config.m_rnn)
        self.d = {k: torch.zeros(s) for k, s in self._device_shapes().items()}
        self._range, self.loaded = None, False


def test_checkpoint_round_trip_and_errors(tmp_path):
    cfg = M.MatchConfig(**SMALL)
    v = M.random_variables(cfg, 3)
    assert set(v) == set(cfg.variable_shapes())
    extra = dict(v, global_step=np.array(7, np.int64))
    extra['text_sketchyscene/embedding/Adam'] = np.zeros_like(v['text_sketchyscene/embedding'])
    prefix = str(tmp_path / 'model-7')
    tf_checkpoint.write_checkpoint(prefix, extra)
    back = tf_checkpoint.read_checkpoint(prefix)
    m = _Host(cfg)
    m.load_dict(back)
    assert all(np.array_equal(m.host[k], v[k]) for k in v)
    p = 'text_sketchyscene/'
    c = cfg
    km = v[p + 'mLSTM/lstm_cell/kernel']
    assert np.array_equal(m.d['m/Kv'].numpy()[:, :c.m_rnn], km[:c.v_emb, :c.m_rnn])
    assert np.array_equal(m.d['m/Ks'].numpy()[:, 32:32 + c.m_rnn], km[c.v_emb + c.w_emb + c.w_rnn:c.v_emb + c.w_emb + c.w_rnn + 8, c.m_rnn:2 * c.m_rnn])
    assert np.array_equal(m.d['m/Kh'].numpy()[:c.m_rnn, 96:96 + c.m_rnn], km[-c.m_rnn:, 3 * c.m_rnn:])
    assert not m.d['m/Kh'].numpy()[c.m_rnn:].any() and not m.d['m/Kl'].numpy()[c.w_rnn:].any()
    assert np.array_equal(m.d['ResNet/group_1/bn_conv1'].numpy(), M.fold_norm(*[v['ResNet/group_1/bn_conv1/' + q] for q in M.NORM_PARTS]))
    # the older cell names
    old = {k.replace('/lstm_cell/kernel', '/lstm_cell/weights').replace('/lstm_cell/bias', '/lstm_cell/biases'): a for k, a in v.items()}
    assert p + 'wLSTM/lstm_cell/weights' in old
    m2 = _Host(cfg)
    m2.load_dict(old)
    assert np.array_equal(m2.d['w/Kh'].numpy(), m.d['w/Kh'].numpy())
    # a missing variable and a wrong shape are named
    miss = dict(v)
    del miss['ResNet/group_3_0/block_add/bn/factor']
    with pytest.raises(ValueError, match='ResNet/group_3_0/block_add/bn/factor'):
        _Host(cfg).load_dict(miss)
    wrong = dict(v)
    wrong[p + 'embedding'] = np.zeros((75, 16), np.float32)
    with pytest.raises(ValueError, match='text_sketchyscene/embedding'):
        _Host(cfg).load_dict(wrong)
    with pytest.raises(ValueError):
        M.resolve_snapshot(str(tmp_path / 'nothing'))
    assert M.resolve_snapshot(prefix) == prefix
    (tmp_path / 'checkpoint').write_text('model_checkpoint_path: "model-7"\n')
    assert M.resolve_snapshot(str(tmp_path)) == prefix


# ------------------------------------------------------------------ the space-to-batch argument
def _s2b(x, r):
    n, h, w, c = x.shape
    return x.reshape(n, h // r, r, w // r, r, c).transpose(0, 2, 4, 1, 3, 5).reshape(n * r * r, h // r, w // r, c)


def _b2s(x, r):
    nb, h, w, c = x.shape
    n = nb // (r * r)
    return x.reshape(n, r, r, h, w, c).transpose(0, 3, 1, 4, 2, 5).reshape(n, h * r, w * r, c)


@pytest.mark.parametrize('hw', [(8, 8), (12, 12), (4, 8)])
def test_atrous_conv_is_the_plain_conv_of_the_sub_images(hw):
    rng = np.random.RandomState(2)
    x, w = rng.randn(2, hw[0], hw[1], 5), rng.randn(3, 3, 5, 6)
    for r in (2, 4):
        direct = O.conv(x, w, 1, r)
        assert np.array_equal(_b2s(_s2b(x, r), r), x)
        assert np.abs(_b2s(O.conv(_s2b(x, r), w), r) - direct).max() < 1e-12
    # the regrouping the model uses: space_to_batch(2) applied to the rate-2 layout serves rate 4, and two batch_to_space(2) undo it
    twice = _s2b(_s2b(x, 2), 2)
    assert np.abs(_b2s(_b2s(O.conv(twice, w), 2), 2) - O.conv(x, w, 1, 4)).max() < 1e-12
    # 1 x 1 convs, norms and adds do not care where a pixel sits
    w1 = rng.randn(1, 1, 5, 6)
    assert np.abs(_b2s(_b2s(O.conv(twice, w1), 2), 2) - O.conv(x, w1)).max() < 1e-12


def test_oracle_same_padding_of_the_stride_2_layers():
    """Even sizes pad at the bottom / right only: the 7 x 7 stride-2 conv reads rows 2 oy - 2 .. 2 oy + 4, the max-pool rows 2 oy ..
    2 oy + 2, the 1 x 1 stride-2 conv row 2 oy."""
    assert O.same_pads(64, 7, 2) == (2, 3) and O.same_pads(32, 3, 2) == (0, 1) and O.same_pads(16, 1, 2) == (0, 0)
    assert O.same_pads(9, 3, 2) == (1, 1) and O.same_pads(8, 9, 1) == (4, 4)
    x = -1.0 - np.arange(36, dtype=np.float64).reshape(1, 6, 6, 1)
    p = O.max_pool(x)
    assert p.shape == (1, 3, 3, 1) and p[0, 2, 2, 0] == x[0, 4, 4, 0] and p[0, 0, 0, 0] == x[0, 0, 0, 0]
    x1 = np.random.RandomState(0).randn(1, 8, 8, 3)
    assert np.array_equal(O.conv(x1, np.ones((1, 1, 3, 1)), 2)[0, :, :, 0], x1[0, ::2, ::2].sum(-1))


def test_oracle_resize_is_the_legacy_form():
    pred = np.arange(6, dtype=np.float64).reshape(2, 3)
    up = O.resize_bilinear_legacy(pred, 12)
    assert up.shape == (12, 12) and up[0, 0] == 0 and up[0, 4] == 1 and up[0, 2] == 0.5
    assert up[0, 11] == 2 and up[0, 9] == 2.0 - 0.0 and up[11, 0] == 3            # the last cell repeats its edge
    assert np.array_equal(O.corner_max(pred, 12)[0, :4], [4, 4, 4, 4]) and O.corner_max(pred, 12)[11, 11] == 5


# ------------------------------------------------------------------ the command line
def _scene_dir(tmp_path, size=64):
    import scipy.io
    from PIL import Image
    d = tmp_path / 'scene'
    for sub in ('sketches', 'inner_masks', 'seg_data'):
        (d / sub).mkdir(parents=True)
    Image.fromarray(np.full((size, size, 3), 255, np.uint8)).save(str(d / 'sketches' / 'a.png'))
    scipy.io.savemat(str(d / 'inner_masks' / 'a.mat'), {'inner_masks': np.zeros((size, size), np.uint8)})
    masks = np.empty(1, dtype=object)
    masks[0] = np.ones((5, 5), np.uint8)
    np.savez(str(d / 'seg_data' / 'a_datas.npz'), pred_masks=masks, pred_boxes=np.array([[1, 1, 5, 5]], np.int32), pred_class_ids=np.array([15]))
    return str(d)


def test_match_main_refuses_bad_arguments_with_nothing_written(tmp_path):
    import match_main
    cfg = M.MatchConfig(**SMALL)
    prefix = str(tmp_path / 'model-1')
    tf_checkpoint.write_checkpoint(prefix, M.random_variables(cfg, 0))
    scene = _scene_dir(tmp_path)
    results = str(tmp_path / 'results')
    good = ['--snapshot', prefix, '--vocab_file', os.path.join(GOLD, 'vocab.txt'), '--scene_dir', scene, '--scene_size', '64',
            '--vocab_size', '76', '--text_len', '15', '--image_id', 'a', '--instruction', 'the house', '--results_dir', results]
    args = match_main.build_parser().parse_args(good)
    match_main.checked_arguments(args)          # the good arguments pass the checks

    def bad(**change):
        argv = list(good)
        for k, val in change.items():
            i = argv.index('--' + k)
            if val is None:
                del argv[i:i + 2]
            else:
                argv[i + 1] = val
        with pytest.raises(ValueError):
            match_main.main(argv)
        assert not os.path.exists(results)
    bad(snapshot=None)
    bad(snapshot=str(tmp_path / 'nothing'))
    bad(image_id=None)
    bad(image_id='b')
    bad(instruction=None)
    bad(instruction=' - ')
    bad(scene_size='72')
    bad(scene_size='0')
    bad(text_len='0')
    bad(vocab_size='75')
    bad(vocab_file=str(tmp_path / 'no_vocab.txt'))
    bad(scene_dir=str(tmp_path / 'no_scene'))
    defaults = match_main.build_parser().parse_args([])
    assert (defaults.vocab_file, defaults.vocab_size, defaults.text_len, defaults.scene_dir, defaults.scene_size, defaults.results_dir) == \
        ('data/match_vocab.txt', 76, 15, 'examples', 768, 'outputs/match_results')
