"""The host side of the matcher's SegNet backbone (MatchConfig(backbone='segnet'), match_main.py --weights segnet; DESIGN.md section
8.12), without a GPU: the variable list, the oracle tests/segnet_oracle.py on its own definitions, the conv bias in front of the
norm, the moving moments through a snapshot, and the command line's refusals -- every one before any device call."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import match_eval_oracle as EO
import segnet_oracle as SO
from sketchyscenecolorization_amd import match_train as T, matching as M, tf_checkpoint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = os.path.join(ROOT, 'tests', 'golden', 'match', 'vocab.txt')
NARROW = dict(v_emb=24, w_emb=16, w_rnn=20, m_rnn=12)
SMALL = dict(size=64, filters=(8, 16, 32, 32, 32), backbone='segnet', **NARROW)

# segnet_model.py:56-95 with is_intermediate: (stage, the output widths of its convs)
RELEASED = [('enc_1', (64, 64)), ('enc_2', (128, 128)), ('enc_3', (256, 256, 256)), ('enc_4', (512, 512, 512)),
            ('enc_5', (512, 512, 512)), ('dec_5', (512, 512, 512)), ('dec_4', (512, 512))]


def _released_list():
    """{name: shape} written out from the reference's scopes: conv<k>/DW, conv<k>/biases, BatchNorm{,_1,_2}/{beta, moving_mean,
    moving_variance}."""
    want, cin = {}, 3
    for stage, widths in RELEASED:
        for k, cout in enumerate(widths):
            want['SegNet/%s/conv%d/DW' % (stage, k + 1)] = (3, 3, cin, cout)
            want['SegNet/%s/conv%d/biases' % (stage, k + 1)] = (cout,)
            norm = 'SegNet/%s/BatchNorm%s' % (stage, ('', '_1', '_2')[k])
            for part in ('beta', 'moving_mean', 'moving_variance'):
                want['%s/%s' % (norm, part)] = (cout,)
            cin = cout
    return want


def test_variable_names_and_shapes():
    cfg = M.MatchConfig(backbone='segnet')
    assert cfg.filters == (64, 128, 256, 512, 512) and cfg.feat_channels == 512 and cfg.feat == 96
    got = {k: tuple(s) for k, s in cfg.variable_shapes().items() if not k.startswith(M.HEAD)}
    want = _released_list()
    assert len([k for k in want if k.endswith('/DW')]) == 18 and len([k for k in want if k.endswith('/beta')]) == 18
    assert got == want, set(got) ^ set(want)
    assert not [k for k in cfg.variable_shapes() if 'gamma' in k or k.startswith('ResNet/')]
    assert want['SegNet/enc_1/conv1/DW'] == (3, 3, 3, 64) and want['SegNet/dec_4/BatchNorm_1/beta'] == (512,)
    assert tuple(cfg.variable_shapes()[M.HEAD + 'visual_feat_projection/DW']) == (1, 1, 512, 1000)
    # the head's variables are those of the DeepLab configuration but for the projection's input width
    head = {k: s for k, s in cfg.variable_shapes().items() if k.startswith(M.HEAD)}
    head_d = {k: s for k, s in M.MatchConfig().variable_shapes().items() if k.startswith(M.HEAD)}
    assert list(head) == list(head_d) and [k for k in head if tuple(head[k]) != tuple(head_d[k])] == [M.HEAD + 'visual_feat_projection/DW']
    # configurable widths: feat is filters[3]
    small = M.MatchConfig(**SMALL)
    assert small.feat_channels == 32 and tuple(small.variable_shapes()['SegNet/dec_5/conv3/DW']) == (3, 3, 32, 32)
    wide = M.MatchConfig(size=64, filters=(8, 16, 32, 48, 64), backbone='segnet')
    assert wide.feat_channels == 48 and tuple(wide.variable_shapes()['SegNet/dec_5/conv3/DW']) == (3, 3, 64, 48)
    assert tuple(wide.variable_shapes()['SegNet/dec_4/conv1/DW']) == (3, 3, 48, 48)


def test_the_default_configuration_is_unchanged():
    c = M.MatchConfig()
    assert (c.backbone, c.size, c.units, c.filters) == ('deeplab', 768, (3, 4, 23, 3), (64, 256, 512, 1024, 2048))
    assert (c.v_emb, c.w_emb, c.w_rnn, c.m_rnn, c.vocab_size, c.max_len, c.use_attn) == (1000, 1000, 1000, 500, 76, 15, False)
    assert c.feat_channels == 2048 and c.feat == 96
    shapes = c.variable_shapes()
    assert not [k for k in shapes if k.startswith('SegNet/')] and 'ResNet/group_5_2/block_3/bn/gamma' in shapes
    assert tuple(shapes['ResNet/group_1/conv1/DW']) == (7, 7, 3, 64) and tuple(shapes[M.HEAD + 'visual_feat_projection/DW']) == (1, 1, 2048, 1000)
    assert T.snapshot_prefix('r', 5) == os.path.join('r', 'deeplab_RMI_iter_5.tfmodel')
    assert T.snapshot_prefix('r', 5, 'segnet') == os.path.join('r', 'segnet_RMI_iter_5.tfmodel')
    with pytest.raises(ValueError, match='fcn_8s'):
        M.MatchConfig(backbone='fcn_8s')


def test_segnet_initial_variables_have_the_parents_bits():
    """profiles/match_backbones_once.txt keeps the digests scripts/match_forward_digest.py --segnet 1 printed on the parent commit's
    tree; its ``host`` lines are random_variables(cfg, 41) of the SegNet cases, which rest on the order of the backbone's
    variables and which every device line of that record starts from.  This tree's are the same."""
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    try:
        import match_forward_digest as D
    finally:
        sys.path.pop(0)
    want = {k: v for k, v in D.recorded(os.path.join(ROOT, 'profiles', 'match_backbones_once.txt')).items() if ' host ' in k}
    got = dict(line for case in D.SEGNET_CASES for line in D.segnet_digests(*case, host_only=True))
    assert len(want) == 5 and set(got) == set(want), set(got) ^ set(want)
    for what, sha in got.items():
        assert sha == want[what], what


def test_a_size_that_is_no_multiple_of_32_is_refused():
    for size in (48, 72, 16, 760):
        with pytest.raises(ValueError, match='multiple of 32'):
            M.MatchConfig(size=size, backbone='segnet')
    with pytest.raises(ValueError, match='multiple of 4'):
        M.MatchConfig(size=64, filters=(8, 16, 30, 32, 32), backbone='segnet')
    assert M.MatchConfig(size=96, backbone='segnet').feat == 12


def test_scratch_memory_is_the_largest_live_pair():
    """At 768 x 768 the largest pair is enc_1's two conv outputs, 768 * 768 * 64 floats each; the codes are one byte per pooled
    element; the refusal names the bytes."""
    cfg = M.MatchConfig(backbone='segnet')
    big = 768 * 768 * 64
    assert cfg.net.scratch_floats() == [big, big]
    codes = 384 * 384 * 64 + 192 * 192 * 128 + 96 * 96 * 256 + 48 * 48 * 512 + 24 * 24 * 512
    need = 4 * (2 * big + 768 * 768 * 4 + 96 * 96 * 512) + codes
    assert cfg.net.scratch_bytes() == need
    assert cfg.net.check_scratch(2 * need) == need
    with pytest.raises(ValueError, match=str(need)):
        cfg.net.check_scratch(2 * need - 2)
    ops = [p[0] for p in cfg.net.plan()]
    assert ops.count('conv') == 18 and ops.count('pool') == 5 and ops.count('unpool') == 2 and ops[-1] == 'act'
    assert [(p[1], p[5], p[6]) for p in cfg.net.plan() if p[0] == 'unpool'] == [('dec_5', 24, 48), ('dec_4', 48, 96)]


# ------------------------------------------------------------------ the oracle on its own definitions
def test_oracle_code_form_equals_the_flat_index_form():
    """max_pool_with_argmax's flat index ((2y + dy) * W + 2x + dx) * C + c at 6 x 10 x 4, against a literal walk over the windows
    that takes the first maximum in row-major order."""
    rng = np.random.RandomState(0)
    x = rng.randn(1, 6, 10, 4)
    x[0, 2:4, 4:6, 1] = 0.7                     # an exact four-way tie, and a two-way one between the second row's taps
    x[0, 0:2, 0:2, 2] = [[-1.0, -2.0], [0.5, 0.5]]
    pooled, ind, code, margin = SO.max_pool_with_argmax(x)
    H, W, C = 6, 10, 4
    for y in range(3):
        for xx in range(5):
            for c in range(C):
                best, at = -np.inf, None
                for dy in (0, 1):
                    for dx in (0, 1):
                        v = x[0, 2 * y + dy, 2 * xx + dx, c]
                        if v > best:
                            best, at = v, ((2 * y + dy) * W + 2 * xx + dx) * C + c
                assert pooled[0, y, xx, c] == best and ind[0, y, xx, c] == at
                assert code[0, y, xx, c] == 2 * ((at // C // W) - 2 * y) + ((at // C) % W - 2 * xx)
                assert x.reshape(-1)[at] == best
    assert code[0, 1, 2, 1] == 0 and margin[0, 1, 2, 1] == 0 and code[0, 0, 0, 2] == 2 and margin[0, 0, 0, 2] == 0
    assert (margin >= 0).all() and (margin > 0).mean() > 0.9
    # given codes are taken instead of the oracle's own
    other = (code + 1) & 3
    p2, ind2, code2, _m = SO.max_pool_with_argmax(x, other)
    assert np.array_equal(code2, other) and np.array_equal(ind2, SO.flat_index(other, W))
    assert np.array_equal(p2.reshape(-1), x.reshape(-1)[ind2.reshape(-1)])


def test_oracle_unpool_of_pool():
    rng = np.random.RandomState(1)
    x = rng.randn(2, 6, 10, 4)
    pooled, ind, code, _margin = SO.max_pool_with_argmax(x)
    up = SO.unpool_2d(pooled, ind, (6, 10))
    assert up.shape == x.shape
    taps = SO.window_taps(up)
    assert ((taps != 0).sum(axis=0) <= 1).all()                     # at most one non-zero per window
    assert np.array_equal(taps.sum(axis=0), pooled)                 # and it is the window's maximum
    assert np.array_equal(up[up != 0], x[up != 0])                  # where it was
    assert np.array_equal(SO.max_pool_with_argmax(np.where(up != 0, up, -np.inf))[0], pooled)


def _case(seed=5):
    cfg = M.MatchConfig(**SMALL)
    v = M.random_variables(cfg, seed)
    rng = np.random.RandomState(seed)
    sk = np.full((64, 64, 3), 255, np.uint8)
    sk[rng.rand(64, 64) < 0.3] = 0
    return cfg, v, sk


def test_the_conv_bias_cancels_in_the_norm():
    """The bias in front of a batch-statistics norm moves the mean by itself and nothing else: in float64 the feature map with the
    biases and without differs by rounding only -- 2^-40 of its largest value leaves six decimal digits above the 2^-53 of one
    operation for the sums of 18 layers."""
    cfg, v, sk = _case()
    assert all(np.abs(v[k]).max() > 0.01 for k in v if k.startswith('SegNet/') and k.endswith('/biases'))
    v64 = {k: a.astype(np.float64) for k, a in v.items()}
    x = SO.O.preprocess(sk)[0][None]
    with_b = SO.backbone(x, v64, cfg.filters)
    without = SO.backbone(x, v64, cfg.filters, with_bias=False)
    assert with_b.shape == (1, 8, 8, 32) and (with_b > 0).any()
    diff = np.abs(with_b - without).max()
    print('bias in front of the norm: max difference %.3e of max %.3e' % (diff, np.abs(with_b).max()))
    assert diff <= 2.0 ** -40 * np.abs(with_b).max()
    # the moving moments are not read either
    moved = dict(v64)
    for k in v64:
        if 'moving_' in k:
            moved[k] = v64[k] * 3 + 1
    assert np.array_equal(SO.backbone(x, moved, cfg.filters), with_b)


def test_moving_moments_round_trip_through_a_snapshot(tmp_path):
    cfg, v, _sk = _case(7)
    moments = [k for k in v if 'moving_' in k]
    assert len(moments) == 36 and all(v[k].any() for k in moments)
    model = M.MatchModel(cfg, device='cpu')
    model.load_dict(v)
    flat = model.flat.clone()
    trainer = T.MatchTrainer(model)
    out = trainer.export_variables()
    assert set(out) == set(v) == set(cfg.variable_shapes())
    for name, a in v.items():
        assert out[name].dtype == np.float32 and np.array_equal(out[name], a), name
    prefix = T.write_snapshot(trainer, str(tmp_path), 2, T.TupleCursor(3, __import__('random').Random(0)))
    assert prefix == str(tmp_path / 'segnet_RMI_iter_2.tfmodel') and T.snapshot_iteration(prefix) == 2
    back = tf_checkpoint.read_checkpoint(prefix)
    for name in v:
        assert np.array_equal(back[name], v[name]), name
    model.flat.zero_()
    model.load_dict(back)
    assert torch.equal(model.flat, flat)
    # a checkpoint without the moving moments loads with their initial values, 0 and 1; the device buffer is the same
    thin = {k: a for k, a in v.items() if 'moving_' not in k}
    model.load_dict(thin)
    assert torch.equal(model.flat, flat)
    assert not model.host['SegNet/enc_3/BatchNorm_2/moving_mean'].any() and (model.host['SegNet/enc_3/BatchNorm_2/moving_variance'] == 1).all()
    # the first filter's three input channels are padded to four on the device, the biases and the moments are not there
    assert tuple(model.d['SegNet/enc_1/conv1/DW'].shape) == (3, 3, 4, 8) and not model.d['SegNet/enc_1/conv1/DW'][:, :, 3].any()
    assert np.array_equal(model.d['SegNet/enc_1/conv1/DW'][:, :, :3].numpy(), v['SegNet/enc_1/conv1/DW'])
    assert not [k for k in model.d if 'biases' in k and k.startswith('SegNet/')] and not [k for k in model.d if 'moving_' in k]
    with pytest.raises(ValueError, match='SegNet/enc_2/conv1/biases'):
        model.load_dict({k: a for k, a in v.items() if k != 'SegNet/enc_2/conv1/biases'})
    model.close()


# ------------------------------------------------------------------ the command line
def _match_files(tmp_path, cfg, variables, name='snap-1'):
    """A snapshot and the flags of --mode match.  The scene's files only have to be there: every refusal held here comes before
    they are read."""
    scene = tmp_path / 'scene'
    for sub, fname in (('sketches', '7.png'), ('inner_masks', '7.mat'), ('seg_data', '7_datas.npz')):
        os.makedirs(str(scene / sub), exist_ok=True)
        (scene / sub / fname).write_bytes(b'')
    prefix = str(tmp_path / name)
    tf_checkpoint.write_checkpoint(prefix, variables)
    return ['--snapshot', prefix, '--vocab_file', VOCAB, '--scene_size', str(cfg.size), '--scene_dir', str(scene), '--image_id', '7',
            '--instruction', 'the bus', '--results_dir', str(tmp_path / 'results')]


def test_command_line_accepts_segnet_and_refuses_the_rest(tmp_path, monkeypatch):
    import match_main
    monkeypatch.setattr(M, 'MatchModel', None)          # anything that reaches the device fails here
    seg = M.MatchConfig(**SMALL)
    deep = M.MatchConfig(size=64, units=(1, 1, 1, 1), filters=(8, 16, 32, 64, 128), **NARROW)
    assert match_main.build_parser().parse_args([]).weights == 'deeplab'
    argv_seg = _match_files(tmp_path, seg, M.random_variables(seg, 2), 'seg-1')
    argv_deep = _match_files(tmp_path, deep, M.random_variables(deep, 2), 'deep-1')
    # accepted, in --mode match and --mode eval's own checks
    cfg = match_main.checked_arguments(match_main.build_parser().parse_args(argv_seg + ['--weights', 'segnet']))[0]
    assert cfg.backbone == 'segnet' and cfg.filters == (64, 128, 256, 512, 512) and match_main.agreed_config(seg, cfg) is seg
    assert match_main.checked_arguments(match_main.build_parser().parse_args(argv_deep))[0].backbone == 'deeplab'
    # the other backbones, in every mode
    for mode in ('match', 'eval', 'train'):
        for other in ('fcn_8s', 'deeplab_v3plus'):
            with pytest.raises(ValueError, match=r'--weights %r.*not built' % other):
                match_main.main(['--mode', mode, '--weights', other] + argv_seg)
    # a snapshot of one backbone under the other's flag: refused from the index alone, naming the flag and a variable
    for mode in ([], ['--mode', 'eval']):
        with pytest.raises(ValueError, match=r'SegNet/dec_4/BatchNorm/beta.*--weights segnet'):
            match_main.main(mode + argv_seg, config=deep)
        with pytest.raises(ValueError, match=r'ResNet/group_1/bn_conv1/beta.*--weights deeplab'):
            match_main.main(mode + argv_deep + ['--weights', 'segnet'], config=seg)
    # a config that disagrees with the flag
    with pytest.raises(ValueError, match='backbone'):
        match_main.main(argv_seg + ['--weights', 'segnet'], config=deep)
    with pytest.raises(ValueError, match='backbone'):
        match_main.agreed_config(seg, match_main.checked_arguments(match_main.build_parser().parse_args(argv_deep))[0])
    # a size that is no multiple of 32
    k = argv_seg.index('--scene_size')
    with pytest.raises(ValueError, match='multiple of 32'):
        match_main.main(argv_seg[:k + 1] + ['80'] + argv_seg[k + 2:] + ['--weights', 'segnet'])
    assert not os.path.exists(str(tmp_path / 'results'))


def test_train_mode_with_segnet(tmp_path, monkeypatch):
    import match_main
    monkeypatch.setattr(M, 'MatchModel', None)
    seg = M.MatchConfig(**SMALL)
    deep = M.MatchConfig(size=64, units=(1, 1, 1, 1), filters=(8, 16, 32, 64, 128), **NARROW)
    v = M.random_variables(seg, 0)
    backbone = str(tmp_path / 'segnet-1')
    tf_checkpoint.write_checkpoint(backbone, {k: a for k, a in v.items() if k.startswith('SegNet/')})
    resnet = str(tmp_path / 'resnet-1')
    tf_checkpoint.write_checkpoint(resnet, {k: a for k, a in M.random_variables(deep, 0).items() if k.startswith('ResNet/')})
    flags = EO.write_split(str(tmp_path), 'train')[:4]
    logs = str(tmp_path / 'log')

    def argv(snaps, bb=backbone, weights='segnet'):
        return ['--mode', 'train', '--backbone_snapshot', bb, '--vocab_file', VOCAB, '--scene_size', '64', '--snapshot_root', snaps,
                '--log_root', logs, '--max_iteration', '4', '--weights', weights] + flags
    none = str(tmp_path / 'none')
    for cache in ('off', 'device', 'features'):
        cfg, _vocab, tuples, resume, bb = match_main.checked_train_arguments(
            match_main.build_parser().parse_args(argv(none) + ['--scene_cache', cache, '--use_attn', '1']))
        assert (cfg.backbone, cfg.use_attn, len(tuples), resume, bb) == ('segnet', True, 6, None, backbone)
    with pytest.raises(ValueError, match=r'--train_backbone 1 --weights segnet.*SegNet backward is not built'):
        match_main.main(argv(none) + ['--train_backbone', '1'], config=seg)
    with pytest.raises(ValueError, match=r'--weights .fcn_8s.'):
        match_main.main(argv(none, weights='fcn_8s'))
    # the backbone's checkpoint of the other kind
    with pytest.raises(ValueError, match=r'ResNet/.*--weights segnet'):
        match_main.main(argv(none, bb=resnet), config=seg)
    with pytest.raises(ValueError, match=r'SegNet/.*--weights deeplab'):
        match_main.main(argv(none, weights='deeplab'), config=deep)
    with pytest.raises(ValueError, match=r'backbone_snapshot.*SegNet/\*'):
        match_main.main([a for a in argv(none) if a not in ('--backbone_snapshot', backbone)])
    # a resume: the snapshot root's segnet_RMI_iter_<n>.tfmodel is found; under --weights deeplab it is refused
    snaps = str(tmp_path / 'snaps')
    os.makedirs(snaps)
    prefix = T.snapshot_prefix(snaps, 2, 'segnet')
    tf_checkpoint.write_checkpoint(prefix, v)
    with open(os.path.join(snaps, 'checkpoint'), 'w') as f:
        f.write('model_checkpoint_path: "segnet_RMI_iter_2.tfmodel"\n')
    with open(prefix + '.train_state.json', 'w') as f:
        json.dump({'cursor': 1, 'order': list(range(6)), 'rng': [3, [0] * 625, None], 'iteration': 2}, f)
    assert match_main.checked_train_arguments(match_main.build_parser().parse_args(argv(snaps)))[3] == prefix
    with pytest.raises(ValueError, match=r'SegNet/.*--weights deeplab'):
        match_main.main(argv(snaps, weights='deeplab'), config=deep)
    assert not os.path.exists(logs) and not os.path.exists(none)
