"""SHA-256 digests of what the matcher computes, inference and training, on the smallest configurations that reach every branch
of its forward pass: both step forms of the LSTM cells (narrow: fp32 with live padding; bf: bf16, where inference passes no
gate buffer), the attention off and on, the head trainer and the backbone trainer (units 2,1,2,2: projection and identity
units, the stride-2 unit, both regroups), snapshots written and resumed.  With every device case goes a digest of the names
that went through ``hip.call`` during it, in order: an added or dropped fill, copy or split shows there.  Run on the parent
commit's tree and on this one,

    python scripts/match_forward_digest.py --tree /path/to/a/built/checkout --tag parent

the lines must be equal: profiles/match_forward_once.txt keeps the parent's, tests/test_gpu_match_train.py holds this tree's
against them (the two ``host`` lines, which need no device: tests/test_match_train.py).  Only what both trees have is used.

``segnet_digests`` (--segnet 1) is the same record for MatchConfig(backbone='segnet'): filters (8, 16, 32, 32, 32) at size 64 with
both head widths and the attention off and on -- the initial variables, inference, the head trainer on the frozen backbone, its
snapshot, a resumed step, the launch names -- and inference alone at size 96, where the last pool reaches an odd 3 x 3 map.
profiles/match_backbones_once.txt keeps the parent's lines; tests/test_gpu_match_segnet.py and tests/test_match_segnet.py hold
this tree's against them."""
import argparse
import hashlib
import os
import sys
import tempfile

SMALL = dict(size=64, units=(1, 1, 1, 1), filters=(8, 16, 32, 64, 128))
WIDTHS = {'narrow': dict(v_emb=24, w_emb=24, w_rnn=40, m_rnn=20), 'bf': dict(v_emb=128, w_emb=128, w_rnn=128, m_rnn=128)}
CASES = [(w, a) for w in ('narrow', 'bf') for a in (0, 1)]
BACKBONE_UNITS = (2, 1, 2, 2)
SEGNET_FILTERS = (8, 16, 32, 32, 32)
SEGNET_CASES = [(w, a, 64) for w, a in CASES] + [('narrow', 0, 96)]       # (widths, use_attn, size); 96: inference only


def case_name(widths, use_attn):
    return '%s attn=%d' % (widths, use_attn)


def _sha(a):
    return hashlib.sha256(a if isinstance(a, bytes) else a.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _config(widths, use_attn, **kw):
    from sketchyscenecolorization_amd import matching
    return matching.MatchConfig(**dict(dict(SMALL, **WIDTHS[widths]), use_attn=bool(use_attn), **kw))


def host_digests(widths, use_attn):
    """-> [(what, sha256)] of the two sets of initial variables; no device."""
    from sketchyscenecolorization_amd import match_train, matching
    cfg = _config(widths, use_attn)
    cat = lambda v: b''.join(v[k].tobytes() for k in v)
    return [('%s host random_variables(41)' % case_name(widths, use_attn), _sha(cat(matching.random_variables(cfg, 41)))),
            ('%s host init_head(5)' % case_name(widths, use_attn), _sha(cat(match_train.init_head(cfg, 5))))]


class _Launches(object):
    """Records the names that go through hip.call while it is active."""

    def __enter__(self):
        from sketchyscenecolorization_amd import hip
        self.names, self.call = [], hip.call

        def call(name, *args, **kw):
            self.names.append(name)
            return self.call(name, *args, **kw)
        hip.call = call
        return self

    def __exit__(self, *exc):
        from sketchyscenecolorization_amd import hip
        hip.call = self.call

    def digest(self):
        return _sha('\n'.join(self.names).encode())


def _train(out, tag, make_trainer, cfg, variables, scene, sentences, resident):
    """Two steps from host arrays (and one from a device-resident scene with its feature map, where the trainer takes one), the
    snapshot they leave, a resumed step on a fresh model."""
    import random
    import numpy as np
    import torch
    from sketchyscenecolorization_amd import match_train, matching, tf_checkpoint
    model = matching.MatchModel(cfg)
    model.load_dict(variables)
    trainer = make_trainer(model)
    lut = match_train.caption_lut([2])
    with _Launches() as rec:
        for idx, L in sentences[:2]:
            trainer.step(scene, lut, idx, L, 2.5e-4)
        if resident:
            feat = model.features(scene['sketch'])[0].clone()
            dev = {'sketch_d': torch.from_numpy(scene['sketch']).cuda(), 'labels_d': torch.from_numpy(scene['labels']).cuda(),
                   'feat_d': feat}
            trainer.step(dev, lut, sentences[2][0], sentences[2][1], 2.0e-4)
        loss = trainer.last_loss()
    out.append((tag + ' steps class loss', _sha(np.float64(loss).tobytes())))
    out.append((tag + ' steps model.flat', _sha(model.flat)))
    for name in ('grad', 'adam_m', 'adam_v', 'b_grad', 'b_adam_m', 'b_adam_v'):
        if hasattr(trainer, name):
            out.append(('%s steps %s' % (tag, name), _sha(getattr(trainer, name))))
    out.append((tag + ' steps launches', rec.digest()))
    with tempfile.TemporaryDirectory() as d:
        prefix = match_train.write_snapshot(trainer, d, trainer.step_count, match_train.TupleCursor(3, random.Random(0)))
        for ext in ('.index', '.data-00000-of-00001'):
            with open(prefix + ext, 'rb') as f:
                out.append(('%s snapshot %s' % (tag, ext), _sha(f.read())))
        tensors = tf_checkpoint.read_checkpoint(prefix)
    model.close()
    model = matching.MatchModel(cfg)
    model.load_dict(tensors)
    trainer = make_trainer(model)
    trainer.load_slots(tensors, int(tensors['Variable']))
    with _Launches() as rec:
        trainer.step(scene, lut, sentences[2][0], sentences[2][1], 1.5e-4)
        trainer.last_loss()
    out.append((tag + ' resumed step model.flat', _sha(model.flat)))
    out.append((tag + ' resumed step launches', rec.digest()))
    model.close()


def _inference_and_head_trainer(out, tag, cfg, variables, train=True):
    """Inference and the head trainer of one configuration into ``out``; -> (scene, the trainers' sentences)."""
    import numpy as np
    import torch
    from sketchyscenecolorization_amd import match_train, matching
    rng = np.random.RandomState(42)
    sk = np.full((cfg.size, cfg.size, 3), 255, np.uint8)
    sk[rng.rand(cfg.size, cfg.size) < 0.5] = 0
    labels = np.zeros((cfg.size, cfg.size), np.uint8)
    labels[4:30, 6:40], labels[34:60, 20:62] = 1, 2
    sentences = []
    for L in (15, 3, 1, 5):
        idx = rng.randint(2, cfg.vocab_size, cfg.max_len)
        idx[L:] = 0
        sentences.append((idx, L))
    # inference: the head after a longer sentence (stale rows behind L), the whole pass, the pass in two halves
    model = matching.MatchModel(cfg)
    model.load_dict(variables)
    feat = torch.from_numpy(np.maximum(rng.randn(1, cfg.feat, cfg.feat, cfg.feat_channels), 0).astype(np.float32)).cuda()
    with _Launches() as rec:
        for idx, L in sentences[:3]:
            out.append(('%s head L=%d pred' % (tag, L), _sha(model.head(feat, torch.from_numpy(idx.astype(np.int32)).cuda(), L))))
        up, predicts = model.forward(sk, *sentences[3])
        out += [(tag + ' forward up', _sha(up)), (tag + ' forward predicts', _sha(predicts))]
        fmap, stroke = model.features(sk)
        out += [(tag + ' features feat', _sha(fmap)), (tag + ' features stroke', _sha(stroke))]
        up, predicts = model.predict(fmap, stroke, *sentences[1])
        out += [(tag + ' predict up', _sha(up)), (tag + ' predict predicts', _sha(predicts))]
    out.append((tag + ' inference launches', rec.digest()))
    model.close()
    scene = {'sketch': sk, 'labels': labels}
    order = [sentences[3], sentences[1], sentences[0]]
    if train:
        _train(out, tag + ' head trainer', match_train.MatchTrainer, cfg, variables, scene, order, True)
    return scene, order


def device_digests(widths, use_attn):
    """-> [(what, sha256)] of one case, from the sketchyscenecolorization_amd that is importable now."""
    from sketchyscenecolorization_amd import match_backbone_train, matching
    tag = case_name(widths, use_attn)
    cfg = _config(widths, use_attn)
    out = []
    scene, order = _inference_and_head_trainer(out, tag, cfg, matching.random_variables(cfg, 41))
    deep = _config(widths, use_attn, units=BACKBONE_UNITS)
    _train(out, tag + ' backbone trainer', match_backbone_train.BackboneMatchTrainer, deep, matching.random_variables(deep, 41), scene,
           order, False)
    return out


def digests(widths, use_attn):
    return host_digests(widths, use_attn) + device_digests(widths, use_attn)


def segnet_case_name(widths, use_attn, size):
    return 'segnet %s attn=%d size=%d' % (widths, use_attn, size)


def segnet_digests(widths, use_attn, size, host_only=False):
    """-> [(what, sha256)] of one SegNet case: the ``host`` line, and unless host_only the device lines."""
    from sketchyscenecolorization_amd import matching
    tag = segnet_case_name(widths, use_attn, size)
    cfg = matching.MatchConfig(size=size, filters=SEGNET_FILTERS, backbone='segnet', use_attn=bool(use_attn), **WIDTHS[widths])
    variables = matching.random_variables(cfg, 41)
    out = [(tag + ' host random_variables(41)', _sha(b''.join(variables[k].tobytes() for k in variables)))]
    if not host_only:
        _inference_and_head_trainer(out, tag, cfg, variables, train=size == 64)
    return out


def recorded(path, tag='parent'):
    """{what: sha256} of the ``tag sha256 <hex> <what>`` lines of a profile file."""
    want = {}
    with open(path) as f:
        for line in f:
            part = line.rstrip('\n').split(' ', 3)
            if len(part) == 4 and part[0] == tag and part[1] == 'sha256':
                want[part[3]] = part[2]
    return want


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument('--tag', default='tree')
    ap.add_argument('--host_only', type=int, default=0, help='1: only the lines that need no device')
    ap.add_argument('--segnet', type=int, default=0, help='1: the cases of segnet_digests in place of the DeepLab ones')
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    if a.segnet:
        cases = [segnet_digests(*case, host_only=bool(a.host_only)) for case in SEGNET_CASES]
    else:
        cases = [(host_digests if a.host_only else digests)(widths, use_attn) for widths, use_attn in CASES]
    for lines in cases:
        for what, sha in lines:
            print('%s sha256 %s %s' % (a.tag, sha, what), flush=True)
