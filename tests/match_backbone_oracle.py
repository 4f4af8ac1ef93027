"""The whole matcher restated in torch on the CPU with every gradient from autograd, for tests/test_match_backbone_train.py and
tests/test_gpu_match_backbone_train.py: the DeepLab-ResNet backbone of deeplab_model.py with frozen norms -- F.conv2d with an
explicit TF SAME padding and ``dilation`` for the atrous convs (a direct dilated conv, not the space-to-batch layout the product
runs), the frozen affine y = a*x + b with a and b worked out in float64 from the five stored parts, F.max_pool2d on an input padded
with -inf after -- then the head and the loss of tests/match_train_oracle.py, and TF's Adam with the l2 regulariser in float64
NumPy.  float64 by default; the same pass in float32 is the yardstick of the device's tolerance.  Nothing of the product is
imported and nothing of its hand-derived backward is here.

RMI_model.py:320-330 with train_fusion_var_only=False: every trainable variable is trained; the norms' beta, gamma, factor, mean
and variance are trainable=False (deeplab_model.py:176-231), so the backbone's share is its ResNet/*/DW filters."""
import numpy as np
import torch
import torch.nn.functional as F

import match_train_oracle as TO
import matching_oracle as MO

EPS = 0.001


def backbone_names(v):
    return [k for k in v if k.startswith('ResNet/') and k.endswith('/DW')]


def trained_names(v, train_backbone=True):
    return (backbone_names(v) if train_backbone else []) + [k for k in TO.HEAD_NAMES if k in v]


def reference_trained_and_regularized(names_trainable, fusion_only):
    """A re-enactment of RMI_model.py:320-330 on (name, trainable) pairs: tvars = the trainable variables, those under
    text_sketchyscene alone when train_fusion_var_only; the regulariser takes the tvars whose name holds 'DW'.
    -> (trained names, regularised names)."""
    tvars = [n for n, trainable in names_trainable if trainable]
    if fusion_only:
        tvars = [n for n in tvars if n.startswith('text_sketchyscene')]
    return tvars, [n for n in tvars if 'DW' in n]


# ------------------------------------------------------------------ layers, NCHW tensors
def fold(v, scope, dtype):
    """[a, b] of the frozen norm in float64 (the product's fold_norm formula), as tensors of ``dtype``."""
    beta, gamma, mean, var = (np.asarray(v[scope + '/' + p], np.float64).reshape(-1) for p in ('beta', 'gamma', 'mean', 'variance'))
    f = float(np.asarray(v[scope + '/factor'], np.float64).reshape(-1)[0])
    a = gamma / np.sqrt(var / f + EPS)
    b = beta - mean / f * a
    return torch.tensor(a, dtype=dtype).view(1, -1, 1, 1), torch.tensor(b, dtype=dtype).view(1, -1, 1, 1)


def conv(x, w, stride=1, rate=1):
    """tf.nn.conv2d(SAME) / tf.nn.atrous_conv2d(SAME): x [N,C,H,W], w [kh,kw,ci,co]."""
    kh, kw = w.shape[:2]
    pt, pb = MO.same_pads(x.shape[2], (kh - 1) * rate + 1, stride)
    pl, pr = MO.same_pads(x.shape[3], (kw - 1) * rate + 1, stride)
    return F.conv2d(F.pad(x, (pl, pr, pt, pb)), w.permute(3, 2, 0, 1), stride=stride, dilation=rate)


def max_pool(x, rec):
    pt, pb = MO.same_pads(x.shape[2], 3, 2)
    pl, pr = MO.same_pads(x.shape[3], 3, 2)
    y, idx = F.max_pool2d(F.pad(x, (pl, pr, pt, pb), value=float('-inf')), 3, 2, return_indices=True)
    rec.append(('pool argmax', idx.numpy().copy()))
    return y


def _relu(x, rec, what):
    rec.append((what, (x.detach() > 0).numpy()))
    assert not bool((x.detach() == 0).any()), what + ': a pre-activation of exactly 0'
    return torch.relu(x)


def backbone(x, t, v, units, filters, rec):
    """x [1,3,S,S]; t {name: tensor} of the filters; v the arrays of the norms -> feat [1,F,S/8,S/8]."""
    dt = x.dtype
    na = lambda y, scope: y * fold(v, scope, dt)[0] + fold(v, scope, dt)[1]
    y = _relu(na(conv(x, t['ResNet/group_1/conv1/DW'], 2), 'ResNet/group_1/bn_conv1'), rec, 'conv1')
    y = max_pool(y, rec)
    for scope, stride, rate in MO.unit_list(units, filters):
        z = _relu(na(conv(y, t[scope + '/block_1/conv/DW'], stride), scope + '/block_1/bn'), rec, scope + '/block_1')
        z = _relu(na(conv(z, t[scope + '/block_2/conv/DW'], 1, rate), scope + '/block_2/bn'), rec, scope + '/block_2')
        z = na(conv(z, t[scope + '/block_3/conv/DW']), scope + '/block_3/bn')
        if scope + '/block_add/conv/DW' in t:
            y = na(conv(y, t[scope + '/block_add/conv/DW'], stride), scope + '/block_add/bn')
        y = _relu(z + y, rec, scope + '/out')
    return y            # group_last's relu of a relu


def tensors(v, dtype, names):
    return {k: torch.tensor(np.asarray(v[k]), dtype=dtype, requires_grad=True) for k in names}


def forward(sketch_u8, t, v, indices, seq_len, units, filters, dtype=torch.float64, rec=None):
    """-> (pred [S/8,S/8], feat [1,S/8,S/8,F]) as tensors on the graph of ``t``."""
    np_dt = np.float64 if dtype == torch.float64 else np.float32
    x, _stroke = MO.preprocess(sketch_u8, np_dt)
    rec = [] if rec is None else rec
    feat = backbone(torch.from_numpy(np.ascontiguousarray(x.transpose(2, 0, 1)[None])), t, v, units, filters, rec)
    feat = feat.permute(0, 2, 3, 1)
    return TO.head(feat, t, indices, seq_len), feat


def loss_and_gradients(sketch_u8, v, indices, seq_len, target, units, filters, dtype=torch.float64, train_backbone=True):
    """-> (class loss, {name: gradient of the class loss} for every trained variable, pred, feat, the record of every relu's sign
    and of the pool's argmax).  With train_backbone=False the backbone's filters are constants."""
    names = trained_names(v, True)
    t = tensors(v, dtype, names)
    if not train_backbone:
        for k in backbone_names(v):
            t[k].requires_grad_(False)
    rec = []
    pred, feat = forward(sketch_u8, t, v, indices, seq_len, units, filters, dtype, rec)
    loss, _up, _live = TO.class_loss(pred, sketch_u8, target, dtype)
    loss.backward()
    grads = {k: (t[k].grad.numpy() if t[k].grad is not None else np.zeros(t[k].shape)) for k in trained_names(v, train_backbone)}
    return float(loss.detach()), grads, pred.detach().numpy(), feat.detach().numpy(), rec


def records_agree(rec_a, rec_b):
    """Every relu sign and every pool argmax of two passes the same -> (bool, the first that differs or None)."""
    assert [w for w, _ in rec_a] == [w for w, _ in rec_b]
    for (what, a), (_w, b) in zip(rec_a, rec_b):
        if not np.array_equal(a, b):
            return False, what
    return True, None


def train(sketch_u8, v, indices, seq_len, target, units, filters, steps, lr, weight_decay=5e-4, train_backbone=True,
          dtype=torch.float64):
    """``steps`` iterations on one tuple: the class loss in front of every update, then l2 + Adam on every trained variable
    -> (losses, the variables after the last update).  float32: the pass in float32, and the variables and the slots rounded to
    float32 after every update (the update itself in float64 NumPy)."""
    v = {k: np.asarray(a, np.float64) for k, a in v.items()}
    names = trained_names(v, train_backbone)
    m = {k: np.zeros_like(v[k]) for k in names}
    s = {k: np.zeros_like(v[k]) for k in names}
    keep = (lambda a: a) if dtype == torch.float64 else (lambda a: a.astype(np.float32).astype(np.float64))
    losses = []
    for step in range(1, steps + 1):
        loss, grads, _p, _f, _r = loss_and_gradients(sketch_u8, v, indices, seq_len, target, units, filters, dtype, train_backbone)
        losses.append(loss)
        for k in names:
            v[k], m[k], s[k] = (keep(a) for a in TO.update(k, v[k], grads[k], m[k], s[k], lr, step, weight_decay))
    return losses, v
