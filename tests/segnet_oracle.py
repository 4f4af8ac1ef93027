"""The matcher's SegNet backbone restated in NumPy (float64 by default, float32 on request), from the definitions of
Instance_Matching/segnet_model.py with is_intermediate=True: 3x3 SAME convs WITH their biases, tf.contrib.layers.batch_norm with
its defaults (is_training, so the biased moments of the one image; no gamma; epsilon 0.001; the moving moments are not read),
relu, tf.nn.max_pool_with_argmax (2x2, stride 2) with its flat int64 index ((2y + dy) * W + 2x + dx) * C + c, and _unpool_2d as
the literal scatter_nd into the flattened output.  Built on tests/matching_oracle.py (conv, relu, head, finish); nothing of the
product is imported and nothing of the reference.

``codes``: {encoder stage: uint8 [1,h,w,C] of 2*dy + dx}: the oracle pools by these instead of by its own maxima (the value it takes
is then the tap the code names), so that two arithmetics can be compared on one choice of positions."""
import numpy as np

import matching_oracle as O

EPS = 0.001
STAGES = ('enc_1', 'enc_2', 'enc_3', 'enc_4', 'enc_5', 'dec_5', 'dec_4')


def stages(filters):
    """[(stage, [(cin, cout)])] of segnet_model.py:56-95; dec_5 ends at enc_4's width, whose codes dec_4's unpool reads."""
    f1, f2, f3, f4, f5 = filters
    return [('enc_1', [(3, f1), (f1, f1)]), ('enc_2', [(f1, f2), (f2, f2)]), ('enc_3', [(f2, f3), (f3, f3), (f3, f3)]),
            ('enc_4', [(f3, f4), (f4, f4), (f4, f4)]), ('enc_5', [(f4, f5), (f5, f5), (f5, f5)]),
            ('dec_5', [(f5, f5), (f5, f5), (f5, f4)]), ('dec_4', [(f4, f4), (f4, f4)])]


def norm_scope(stage, k):
    return 'SegNet/%s/BatchNorm%s' % (stage, '' if k == 0 else '_%d' % k)


def batch_norm(x, beta):
    """tf.contrib.layers.batch_norm(x) in training mode: tf.nn.moments over N, H, W (biased), scale=False, epsilon 0.001."""
    mean = x.mean(axis=(0, 1, 2))
    var = ((x - mean) ** 2).mean(axis=(0, 1, 2))
    return (x - mean) / np.sqrt(var + x.dtype.type(EPS)) + beta


def conv_bn_relu(x, v, stage, k, with_bias=True):
    scope = 'SegNet/%s/conv%d' % (stage, k + 1)
    y = O.conv(x, v[scope + '/DW'], bias=v[scope + '/biases'] if with_bias else None)
    return O.relu(batch_norm(y, v[norm_scope(stage, k) + '/beta']))


def window_taps(x):
    """x [N,H,W,C] -> [4,N,H/2,W/2,C]: tap 2*dy + dx of every 2x2 window."""
    return np.stack([x[:, dy::2, dx::2] for dy in (0, 1) for dx in (0, 1)])


def flat_index(code, W):
    """The code 2*dy + dx of every pooled element [N,h,w,C] -> TF's flat index into one image [H*W*C] (include_batch_in_index
    False): ((2y + dy) * W + 2x + dx) * C + c."""
    n, h, w, c = code.shape
    y, x, ch = np.meshgrid(np.arange(h), np.arange(w), np.arange(c), indexing='ij')
    code = code.astype(np.int64)
    return ((2 * y + code // 2) * W + 2 * x + code % 2) * c + ch


def max_pool_with_argmax(x, code=None):
    """-> (pooled [N,H/2,W/2,C], flat int64 index of every pooled element, code uint8, margin = the largest tap minus the second
    largest).  Of equal taps the first in row-major order is taken (np.argmax's rule, and TF's).  code given: the tap it names."""
    n, H, W, c = x.shape
    assert H % 2 == 0 and W % 2 == 0
    taps = window_taps(x)
    own = np.argmax(taps, axis=0).astype(np.uint8)
    srt = np.sort(taps, axis=0)
    margin = srt[3] - srt[2]
    code = own if code is None else np.asarray(code, np.uint8) & 3
    pooled = np.take_along_axis(taps, code[None].astype(np.int64), axis=0)[0]
    return pooled, flat_index(code, W), code, margin


def unpool_2d(pool, ind, out_hw):
    """_unpool_2d: scatter_nd of the pooled values to [batch, flat index] of a zero [N, H*W*C], reshaped."""
    n, h, w, c = pool.shape
    H, W = out_hw
    flat = np.zeros((n, H * W * c), dtype=pool.dtype)
    for b in range(n):
        np.add.at(flat[b], ind[b].reshape(-1), pool[b].reshape(-1))         # scatter_nd adds duplicates; there are none
    return flat.reshape(n, H, W, c)


def backbone(x, v, filters, codes=None, with_bias=True, record=None):
    """x [1,S,S,3] -> the feature [1,S/8,S/8,filters[3]].  record: a dict that receives per encoder stage 'code', 'margin', 'taps'
    (the four taps of every window) and 'pooled'."""
    ind, size = {}, {}
    for stage, convs in stages(filters):
        if stage.startswith('dec'):
            enc = 'enc_' + stage[4:]
            x = unpool_2d(x, ind[enc], size[enc])           # the reference's [48, 48] / [96, 96] at 768
        for k in range(len(convs)):
            x = conv_bn_relu(x, v, stage, k, with_bias)
        if stage.startswith('enc'):
            size[stage] = x.shape[1:3]
            taps = window_taps(x)
            x, ind[stage], code, margin = max_pool_with_argmax(x, None if codes is None else codes[stage])
            if record is not None:
                record[stage] = dict(code=code, margin=margin, taps=taps, pooled=x)
    return x


def sure_windows(rec64, rec32):
    """The records of a float64 and a float32 pass -> {stage: (sure, positive)}: a window is sure when its float64 margin is more
    than 4 x the largest float32-versus-float64 difference among its four taps and its maximum is above that difference;
    positive: its float64 maximum is above 0 (the others pool to 0 whatever the code)."""
    out = {}
    for stage, r in rec64.items():
        diff = np.abs(rec32[stage]['taps'].astype(np.float64) - r['taps']).max(axis=0)
        out[stage] = ((r['margin'] > 4 * diff) & (r['pooled'] > diff), r['pooled'] > 0)
    return out


def unsure_share(sure):
    """The share of the windows with a positive maximum that are not sure, over all stages."""
    n = sum(int(pos.sum()) for _s, pos in sure.values())
    return sum(int((pos & ~s).sum()) for s, pos in sure.values()) / float(n)


def forward(sketch_u8, v, indices, seq_len, filters, T, dtype=np.float64, codes=None, with_bias=True, record=None):
    """-> (up [S,S], predicts uint8 [S,S], pred [S/8,S/8], feat) with every variable and every step in ``dtype``."""
    v = {k: np.asarray(a, dtype=dtype) for k, a in v.items()}
    x, stroke = O.preprocess(sketch_u8, dtype)
    feat = backbone(x[None], v, filters, codes, with_bias, record)
    pred = O.head(feat, v, indices, seq_len, T)
    up, predicts = O.finish(pred, stroke, sketch_u8.shape[0])
    return up, predicts, pred, feat
