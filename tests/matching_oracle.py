"""The instance matcher restated in NumPy (float64 by default), from the definitions of Instance_Matching/RMI_model.py (eval,
fusion 'RMI', no attention), deeplab_model.py (is_intermediate, frozen norms), Pipeline_utils/fg_matching_utils.py and
data_processing/sketch_data_processing.py::get_pred_instance_mask.  Nothing of the product is imported and nothing of the
reference: the convs are torch.nn.functional.conv2d on the CPU with an explicit TF SAME padding and ``dilation`` for the atrous
ones -- a direct dilated conv, not the rearrangement the product uses.

Every function takes ``dtype``: np.float64 for the oracle, np.float32 for the yardstick of the whole-model test (the reference's
own arithmetic, in one more summation order)."""
import re

import numpy as np
import torch
import torch.nn.functional as F

MU = (104.00698793, 116.66876762, 122.67891434)
EPS = 0.001


# ------------------------------------------------------------------ text, spatial table
def tokens(text):
    words = [w.lower() for w in re.split(r'(\W+)', text.strip()) if len(w.strip()) > 0 and w != '-']
    if words and words[-1] == '.':
        words = words[:-1]
    return words


def sentence(text, vocab, T):
    idx = [vocab.get(w, vocab['<unk>']) for w in tokens(text)][:T]
    return idx + [vocab['<pad>']] * (T - len(idx)), len(idx)


def spatial(h, w):
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing='ij')
    xmin, xmax, ymin, ymax = xs / w * 2 - 1, (xs + 1) / w * 2 - 1, ys / h * 2 - 1, (ys + 1) / h * 2 - 1
    return np.stack([xmin, ymin, xmax, ymax, (xmin + xmax) / 2, (ymin + ymax) / 2, np.full_like(xs, 1 / w), np.full_like(xs, 1 / h)],
                    axis=2).astype(np.float32)


# ------------------------------------------------------------------ image
def preprocess(sketch_u8, dtype=np.float64):
    """-> (x [S,S,3] = byte - mu on the channels in RGB order, stroke uint8 [S,S] = 1 where the first byte is not 255: the
    reference sets 0 -> 1 and then 255 -> 0, and only ever asks whether the entry is zero)."""
    x = sketch_u8.astype(dtype) - np.asarray(MU, dtype=dtype)
    return x, (sketch_u8[:, :, 0] != 255).astype(np.uint8)


# ------------------------------------------------------------------ layers (NHWC arrays)
def same_pads(size, k_eff, stride):
    out = -(-size // stride)
    total = max((out - 1) * stride + k_eff - size, 0)
    return total // 2, total - total // 2


def conv(x, w, stride=1, rate=1, bias=None):
    """tf.nn.conv2d(SAME) / tf.nn.atrous_conv2d(SAME): x [N,H,W,C], w [kh,kw,ci,co]."""
    kh, kw = w.shape[:2]
    pt, pb = same_pads(x.shape[1], (kh - 1) * rate + 1, stride)
    pl, pr = same_pads(x.shape[2], (kw - 1) * rate + 1, stride)
    t = F.pad(torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2))), (pl, pr, pt, pb))
    y = F.conv2d(t, torch.from_numpy(np.ascontiguousarray(w.transpose(3, 2, 0, 1))), stride=stride, dilation=rate)
    y = y.numpy().transpose(0, 2, 3, 1)
    return y if bias is None else y + bias


def norm(x, v, scope):
    """The frozen norm as the reference writes it."""
    f = v[scope + '/factor'].reshape(-1)[0]
    mean, var = v[scope + '/mean'] / f, v[scope + '/variance'] / f
    return (x - mean) / np.sqrt(var + x.dtype.type(EPS)) * v[scope + '/gamma'] + v[scope + '/beta']


def relu(x):
    return np.maximum(x, 0)


def max_pool(x):
    """3x3 stride 2 SAME; padded taps are -inf."""
    n, h, w, c = x.shape
    (pt, pb), (pl, pr) = same_pads(h, 3, 2), same_pads(w, 3, 2)
    p = np.full((n, h + pt + pb, w + pl + pr, c), -np.inf, dtype=x.dtype)
    p[:, pt:pt + h, pl:pl + w] = x
    oh, ow = -(-h // 2), -(-w // 2)
    out = np.full((n, oh, ow, c), -np.inf, dtype=x.dtype)
    for ky in range(3):
        for kx in range(3):
            out = np.maximum(out, p[:, ky:ky + 2 * oh:2, kx:kx + 2 * ow:2][:, :oh, :ow])
    return out


def unit(x, v, scope, stride, rate):
    y = relu(norm(conv(x, v[scope + '/block_1/conv/DW'], stride), v, scope + '/block_1/bn'))
    y = relu(norm(conv(y, v[scope + '/block_2/conv/DW'], 1, rate), v, scope + '/block_2/bn'))
    y = norm(conv(y, v[scope + '/block_3/conv/DW']), v, scope + '/block_3/bn')
    if scope + '/block_add/conv/DW' in v:
        x = norm(conv(x, v[scope + '/block_add/conv/DW'], stride), v, scope + '/block_add/bn')
    return relu(y + x)


def unit_list(units, filters):
    out = []
    for g, (n, stride, rate) in enumerate(zip(units, (1, 2, 1, 1), (1, 1, 2, 4))):
        for i in range(n):
            out.append(('ResNet/group_%d_%d' % (g + 2, i), stride if i == 0 else 1, rate))
    return out


def backbone(x, v, units, filters):
    y = relu(norm(conv(x, v['ResNet/group_1/conv1/DW'], 2), v, 'ResNet/group_1/bn_conv1'))
    y = max_pool(y)
    for scope, stride, rate in unit_list(units, filters):
        y = unit(y, v, scope, stride, rate)
    return relu(y)


# ------------------------------------------------------------------ head
def sigmoid(x):
    return 1 / (1 + np.exp(-x))


def l2norm(x):
    return x / np.sqrt(np.maximum((x * x).sum(axis=-1, keepdims=True), x.dtype.type(1e-12)))


def lstm_cell(x, c, h, kernel, bias):
    """tf.nn.rnn_cell.LSTMCell with its defaults: kernel [inputs + C, 4C], gates i, j, f, o, forget bias 1."""
    z = np.concatenate([x, h], axis=1) @ kernel + bias
    i, j, f, o = np.split(z, 4, axis=1)
    c1 = c * sigmoid(f + 1) + sigmoid(i) * np.tanh(j)
    return c1, np.tanh(c1) * sigmoid(o)


def squash(h):
    return relu(0.5 * (np.log(h.dtype.type(1 + 1e-3) + h) - np.log(h.dtype.type(1 + 1e-3) - h)))


def head(feat, v, indices, seq_len, T):
    """feat [1,h,w,F] -> pred [h,w].  dynamic_rnn with sequence_length: the steps t >= seq_len leave the state (and give zero
    outputs, which nothing live reads)."""
    p = 'text_sketchyscene/'
    dt = feat.dtype
    _, fh, fw, _ = feat.shape
    R = fh * fw
    vis = l2norm(conv(feat, v[p + 'visual_feat_projection/DW'], bias=v[p + 'visual_feat_projection/biases'])).reshape(R, -1)
    sp = spatial(fh, fw).reshape(R, 8).astype(dt)
    emb = v[p + 'embedding'][np.asarray(indices)]
    kw, bw = v[p + 'wLSTM/lstm_cell/kernel'], v[p + 'wLSTM/lstm_cell/bias']
    km, bm = v[p + 'mLSTM/lstm_cell/kernel'], v[p + 'mLSTM/lstm_cell/bias']
    cw, cm = bw.shape[0] // 4, bm.shape[0] // 4
    c, h = np.zeros((1, cw), dt), np.zeros((1, cw), dt)
    w_out = np.zeros((T, cw), dt)
    for t in range(seq_len):
        c, h = lstm_cell(emb[t:t + 1], c, h, kw, bw)
        w_out[t] = h[0]
    lang = l2norm(w_out)
    c, h = np.zeros((R, cm), dt), np.zeros((R, cm), dt)
    for t in range(seq_len):
        x = np.concatenate([vis, np.repeat(emb[t:t + 1], R, 0), np.repeat(lang[t:t + 1], R, 0), sp], axis=1)
        c, h = lstm_cell(x, c, h, km, bm)
    out = squash(h) @ v[p + 'm_lstm_output_projection/DW'].reshape(cm, 1) + v[p + 'm_lstm_output_projection/biases']
    return out.reshape(fh, fw)


# ------------------------------------------------------------------ finish
def resize_bilinear_legacy(pred, S, dtype=None):
    """tf.image.resize_bilinear, align_corners=False, the legacy (not half-pixel) form."""
    dt = np.dtype(dtype or pred.dtype)
    h, w = pred.shape

    def axis(n_in):
        src = np.arange(S, dtype=dt) * (dt.type(n_in) / dt.type(S))
        lo = np.floor(src).astype(np.int64)
        return lo, np.minimum(lo + 1, n_in - 1), (src - lo).astype(dt)
    ylo, yhi, wy = axis(h)
    xlo, xhi, wx = axis(w)
    p = pred.astype(dt)
    top = p[ylo][:, xlo] + (p[ylo][:, xhi] - p[ylo][:, xlo]) * wx[None, :]
    bot = p[yhi][:, xlo] + (p[yhi][:, xhi] - p[yhi][:, xlo]) * wx[None, :]
    return top + (bot - top) * wy[:, None]


def corner_max(pred, S):
    """max |corner| of the four values every upsampled pixel is mixed from."""
    h, w = pred.shape
    ylo = np.arange(S) * h // S
    xlo = np.arange(S) * w // S
    yhi, xhi = np.minimum(ylo + 1, h - 1), np.minimum(xlo + 1, w - 1)
    a = np.abs(pred)
    return np.maximum(np.maximum(a[ylo][:, xlo], a[ylo][:, xhi]), np.maximum(a[yhi][:, xlo], a[yhi][:, xhi]))


def finish(pred, stroke, S):
    up = resize_bilinear_legacy(pred, S)
    return up, ((up >= 1e-9) & (stroke != 0)).astype(np.uint8)


def forward(sketch_u8, v, indices, seq_len, units, filters, T, dtype=np.float64):
    """-> (up [S,S], predicts uint8 [S,S], pred [S/8,S/8]) with every variable and every step in ``dtype``."""
    v = {k: np.asarray(a, dtype=dtype) for k, a in v.items()}
    x, stroke = preprocess(sketch_u8, dtype)
    pred = head(backbone(x[None], v, units, filters), v, indices, seq_len, T)
    up, predicts = finish(pred, stroke, sketch_u8.shape[0])
    return up, predicts, pred


# ------------------------------------------------------------------ selection
def occupancy(predicts, boxes, masks):
    """Per instance (sum of predicts AND mask over the box, sum of the mask's bytes) -- get_pred_instance_mask lays the small
    mask into an empty image at its box, so nothing outside the box counts."""
    out = np.zeros((len(masks), 2), dtype=np.int64)
    for k, ((y1, x1, y2, x2), m) in enumerate(zip(np.asarray(boxes).tolist(), masks)):
        out[k] = (np.logical_and(predicts[y1:y2 + 1, x1:x2 + 1], m).sum(), m.astype(np.int64).sum())
    return out


def select(counts, thresh=0.5):
    with np.errstate(divide='ignore', invalid='ignore'):
        scores = counts[:, 0].astype(np.float64) / counts[:, 1].astype(np.float64)
    return [int(k) for k in np.nonzero(scores > thresh)[0]], scores
