"""Training the matcher's fusion head restated in torch on the CPU (float64 by default, float32 as the yardstick of the device's
tolerance), for tests/test_match_train.py and tests/test_gpu_match_train.py: the head of tests/matching_oracle.py::head, the legacy
bilinear resize as a matrix built from matching_oracle.resize_bilinear_legacy's index rule, the summed sigmoid cross entropy over
the pixels whose first sketch byte is <= 104 (Instance_Matching/utils/loss.py, RMI_model.py with training_ignore_bg), TF's Adam
and polynomial_decay in float64 NumPy.  Gradients come from autograd: nothing of the product's hand-written backward is here, and
nothing of the product is imported."""
import numpy as np
import torch

import matching_oracle as MO

P = 'text_sketchyscene/'
HEAD_NAMES = [P + n for n in ('visual_feat_projection/DW', 'visual_feat_projection/biases', 'embedding', 'wLSTM/lstm_cell/kernel',
                              'wLSTM/lstm_cell/bias', 'mLSTM/lstm_cell/kernel', 'mLSTM/lstm_cell/bias',
                              'm_lstm_output_projection/DW', 'm_lstm_output_projection/biases')]
LIVE_MAX = 104


# ------------------------------------------------------------------ the resize as a matrix
def resize_matrix(n_in, S, dtype=np.float64):
    """A [S, n_in] with up = A_y @ pred @ A_x^T: src = dst * (in / out), lower = floor(src), upper = min(lower + 1, in - 1)."""
    dt = np.dtype(dtype)
    src = np.arange(S, dtype=dt) * (dt.type(n_in) / dt.type(S))
    lo = np.floor(src).astype(np.int64)
    hi = np.minimum(lo + 1, n_in - 1)
    w = (src - lo).astype(dt)
    A = np.zeros((S, n_in), dt)
    np.add.at(A, (np.arange(S), lo), 1 - w)
    np.add.at(A, (np.arange(S), hi), w)
    return A


# ------------------------------------------------------------------ the head in torch
def _l2norm(x):
    return x / torch.sqrt(torch.clamp((x * x).sum(dim=-1, keepdim=True), min=1e-12))


def _cell(x, c, h, kernel, bias):
    z = torch.cat([x, h], dim=1) @ kernel + bias
    i, j, f, o = torch.chunk(z, 4, dim=1)
    c1 = c * torch.sigmoid(f + 1) + torch.sigmoid(i) * torch.tanh(j)
    return c1, torch.tanh(c1) * torch.sigmoid(o)


def _squash(h):
    return torch.relu(0.5 * (torch.log((1 + 1e-3) + h) - torch.log((1 + 1e-3) - h)))


def head(feat, v, indices, seq_len):
    """feat tensor [1,h,w,F], v {name: tensor} -> pred [h,w]; MO.head's arithmetic."""
    _, fh, fw, F = feat.shape
    R = fh * fw
    dt = feat.dtype
    vis = _l2norm(feat.reshape(R, F) @ v[P + 'visual_feat_projection/DW'].reshape(F, -1) + v[P + 'visual_feat_projection/biases'])
    sp = torch.from_numpy(MO.spatial(fh, fw).reshape(R, 8)).to(dt)
    emb = v[P + 'embedding'][torch.as_tensor(np.asarray(indices, dtype=np.int64))]
    kw, bw = v[P + 'wLSTM/lstm_cell/kernel'], v[P + 'wLSTM/lstm_cell/bias']
    km, bm = v[P + 'mLSTM/lstm_cell/kernel'], v[P + 'mLSTM/lstm_cell/bias']
    cw, cm = bw.shape[0] // 4, bm.shape[0] // 4
    c, h = torch.zeros((1, cw), dtype=dt), torch.zeros((1, cw), dtype=dt)
    outs = []
    for t in range(seq_len):
        c, h = _cell(emb[t:t + 1], c, h, kw, bw)
        outs.append(h)
    lang = _l2norm(torch.cat(outs, dim=0))
    c, h = torch.zeros((R, cm), dtype=dt), torch.zeros((R, cm), dtype=dt)
    for t in range(seq_len):
        x = torch.cat([vis, emb[t:t + 1].expand(R, -1), lang[t:t + 1].expand(R, -1), sp], dim=1)
        c, h = _cell(x, c, h, km, bm)
    out = _squash(h) @ v[P + 'm_lstm_output_projection/DW'].reshape(cm, 1) + v[P + 'm_lstm_output_projection/biases']
    return out.reshape(fh, fw)


# ------------------------------------------------------------------ the loss
def live_of(sketch_u8):
    return sketch_u8[:, :, 0] <= LIVE_MAX


def class_loss(pred, sketch_u8, target, dtype=torch.float64):
    """pred tensor [h,w]; sketch uint8 [S,S,3]; target bool [S,S] -> (loss, up, live count)."""
    S = sketch_u8.shape[0]
    np_dt = np.float64 if dtype == torch.float64 else np.float32
    Ay = torch.from_numpy(resize_matrix(pred.shape[0], S, np_dt))
    Ax = torch.from_numpy(resize_matrix(pred.shape[1], S, np_dt))
    up = Ay @ pred @ Ax.T
    live = torch.from_numpy(live_of(sketch_u8))
    z = torch.from_numpy(np.asarray(target != 0)).to(dtype)
    per = torch.clamp(up, min=0) - up * z + torch.log1p(torch.exp(-torch.abs(up)))
    return (per * live.to(dtype)).sum(), up, int(live.sum())


def dpred_closed_form(pred, sketch_u8, target):
    """A_y^T ((sigmoid(up) - z) * live) A_x in float64 NumPy."""
    S = sketch_u8.shape[0]
    pred = np.asarray(pred, np.float64)
    Ay, Ax = resize_matrix(pred.shape[0], S), resize_matrix(pred.shape[1], S)
    up = Ay @ pred @ Ax.T
    g = (1 / (1 + np.exp(-up)) - (np.asarray(target) != 0)) * live_of(sketch_u8)
    return Ay.T @ g @ Ax


def loss_on_pred(pred_np, sketch_u8, target, dtype=torch.float64):
    """-> (loss, live, dpred by autograd) for a given pred array."""
    p = torch.tensor(np.asarray(pred_np), dtype=dtype, requires_grad=True)
    loss, _up, live = class_loss(p, sketch_u8, target, dtype)
    loss.backward()
    return float(loss.detach()), live, p.grad.numpy()


def _tensors(v, dtype, grad=True):
    return {k: torch.tensor(np.asarray(a), dtype=dtype, requires_grad=grad) for k, a in v.items() if k in HEAD_NAMES}


def head_gradients(feat_np, v, indices, seq_len, dpred_np, dtype=torch.float64):
    """The gradient of sum(pred * dpred) on every head variable, by autograd -> ({name: array}, pred array)."""
    t = _tensors(v, dtype)
    pred = head(torch.tensor(np.asarray(feat_np), dtype=dtype), t, indices, seq_len)
    (pred * torch.tensor(np.asarray(dpred_np), dtype=dtype)).sum().backward()
    return {k: (a.grad.numpy() if a.grad is not None else np.zeros(a.shape)) for k, a in t.items()}, pred.detach().numpy()


def train_step_loss(feat_np, v, indices, seq_len, sketch_u8, target, dtype=torch.float64):
    """-> (class loss, {name: gradient of the class loss}, pred)."""
    t = _tensors(v, dtype)
    pred = head(torch.tensor(np.asarray(feat_np), dtype=dtype), t, indices, seq_len)
    loss, _up, _live = class_loss(pred, sketch_u8, target, dtype)
    loss.backward()
    return float(loss.detach()), {k: (a.grad.numpy() if a.grad is not None else np.zeros(a.shape)) for k, a in t.items()}, pred.detach().numpy()


# ------------------------------------------------------------------ the optimiser
def polynomial_decay(step, start=2.5e-4, end=1e-5, decay_steps=75000, power=0.9):
    s = min(float(step), float(decay_steps))
    return (start - end) * (1 - s / decay_steps) ** power + end


def adam_tf(var, grad, m, v, lr, t, beta1=0.9, beta2=0.999, eps=1e-8):
    """tf.train.AdamOptimizer's dense apply for its t-th update (t >= 1), float64 -> (var, m, v)."""
    var, grad, m, v = (np.asarray(a, np.float64) for a in (var, grad, m, v))
    lr_t = lr * np.sqrt(1 - beta2 ** t) / (1 - beta1 ** t)
    m = beta1 * m + (1 - beta1) * grad
    v = beta2 * v + (1 - beta2) * grad * grad
    return var - lr_t * m / (np.sqrt(v) + eps), m, v


def update(name, var, grad, m, v, lr, t, weight_decay=5e-4):
    """One update of a head variable from the gradient of the class loss: + weight_decay * var where the name contains 'DW',
    x 2 where it contains 'biases', then Adam."""
    g = np.asarray(grad, np.float64)
    if 'DW' in name:
        g = g + weight_decay * np.asarray(var, np.float64)
    if 'biases' in name:
        g = 2 * g
    return adam_tf(var, g, m, v, lr, t)


def reference_order(tuples, seed, iterations, augment):
    """A plain re-enactment of the reference's loop: random.seed(K), an index array shuffled when the cursor wraps to 0, one
    augmented caption per iteration.  ``augment(caption, random)`` -> the caption with its attribute.  -> [(index, caption)]."""
    import random
    random.seed(seed)
    order = np.arange(len(tuples))
    cur, out = -1, []
    for _ in range(iterations):
        cur = (cur + 1) % len(tuples)
        if cur == 0:
            random.shuffle(order)
        k = int(order[cur])
        out.append((k, augment(tuples[k][1], random)))
    return out
