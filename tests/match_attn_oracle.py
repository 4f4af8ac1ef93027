"""The matcher's head with the model class's word attention (Instance_Matching/RMI_model.py:202-222, use_attn, batch_size 1)
restated in torch on the CPU, on top of tests/match_train_oracle.py: float64 by default, float32 as the yardstick of the device's
tolerance, every gradient from autograd.  Nothing of the product's hand-derived backward is here, and nothing of the product is
imported.

    logit[t] = w_out[t] . DW + b for all T = max_len positions; dynamic_rnn's outputs past the sequence length are zero, so the
               padded positions' logit is b
    attn     = softmax(logit) over ALL T positions: the real words' weights sum to less than 1 whenever L < T
    m_last_h = sum_t attn[t] * m_out[t]; m_out[t] is zero past the sequence length
    pred     = squash(m_last_h) . proj + bias, as without attention

``transcription`` is a second, literal NumPy form of lines 205-217 (tiled weights, a batched [R,1,T] x [R,T,m_rnn] product) that
tests/test_match_attn.py holds the first against."""
import numpy as np
import torch

import match_train_oracle as TO
import matching_oracle as MO

P = TO.P
ATTN_NAMES = [P + 'attn_fc/DW', P + 'attn_fc/biases']
HEAD_NAMES = TO.HEAD_NAMES + ATTN_NAMES


def head(feat, v, indices, seq_len, max_len, use_attn=True, parts=None):
    """feat tensor [1,h,w,F], v {name: tensor} -> pred [h,w].  Without use_attn: match_train_oracle.head's operations in its
    order.  parts: a dict that receives w_output [T,w_rnn], m_output [R,T,m_rnn], attn [T] and m_last_h [R,m_rnn]."""
    _, fh, fw, F = feat.shape
    R, T, L = fh * fw, int(max_len), int(seq_len)
    dt = feat.dtype
    vis = TO._l2norm(feat.reshape(R, F) @ v[P + 'visual_feat_projection/DW'].reshape(F, -1) + v[P + 'visual_feat_projection/biases'])
    sp = torch.from_numpy(MO.spatial(fh, fw).reshape(R, 8)).to(dt)
    emb = v[P + 'embedding'][torch.as_tensor(np.asarray(indices, dtype=np.int64))]
    kw, bw = v[P + 'wLSTM/lstm_cell/kernel'], v[P + 'wLSTM/lstm_cell/bias']
    km, bm = v[P + 'mLSTM/lstm_cell/kernel'], v[P + 'mLSTM/lstm_cell/bias']
    cw, cm = bw.shape[0] // 4, bm.shape[0] // 4
    c, h = torch.zeros((1, cw), dtype=dt), torch.zeros((1, cw), dtype=dt)
    outs = []
    for t in range(L):
        c, h = TO._cell(emb[t:t + 1], c, h, kw, bw)
        outs.append(h)
    lang = TO._l2norm(torch.cat(outs, dim=0))
    c, h = torch.zeros((R, cm), dtype=dt), torch.zeros((R, cm), dtype=dt)
    m_outs = []
    for t in range(L):
        x = torch.cat([vis, emb[t:t + 1].expand(R, -1), lang[t:t + 1].expand(R, -1), sp], dim=1)
        c, h = TO._cell(x, c, h, km, bm)
        m_outs.append(h)
    if use_attn:
        w_output = torch.cat(outs + [torch.zeros((T - L, cw), dtype=dt)], dim=0)                   # [T, w_rnn], zero past L
        m_output = torch.stack(m_outs + [torch.zeros((R, cm), dtype=dt)] * (T - L), dim=1)         # [R, T, m_rnn], zero past L
        logit = (w_output @ v[P + 'attn_fc/DW'] + v[P + 'attn_fc/biases']).reshape(T)
        attn = torch.softmax(logit, dim=0)
        h = (attn.reshape(1, T, 1) * m_output).sum(dim=1)
        if parts is not None:
            parts.update(w_output=w_output.detach().numpy(), m_output=m_output.detach().numpy(), attn=attn.detach().numpy(),
                         m_last_h=h.detach().numpy())
    out = TO._squash(h) @ v[P + 'm_lstm_output_projection/DW'].reshape(cm, 1) + v[P + 'm_lstm_output_projection/biases']
    return out.reshape(fh, fw)


def transcription(w_output, m_output, DW, b):
    """RMI_model.py:205-217 with batch_size 1, line by line in NumPy: w_output [T, w_rnn] (max_len rows, zero past the sequence
    length), m_output [R, T, m_rnn] -> (attn [1, T], m_last_h [R, m_rnn])."""
    w_output, m_output, DW, b = (np.asarray(a, np.float64) for a in (w_output, m_output, DW, b))
    N, (T, cw), R = 1, w_output.shape, m_output.shape[0]
    scores = np.matmul(w_output.reshape(N * T, cw), DW) + b                      # the fully connected layer: [N * T, 1]
    scores = scores.reshape(N, T)
    e = np.exp(scores - scores.max(axis=-1, keepdims=True))
    attn = e / e.sum(axis=-1, keepdims=True)                                    # the softmax over the last axis, all T positions
    tiled = np.tile(attn.reshape(N, 1, 1, T), [1, R, 1, 1]).reshape(-1, 1, T)   # one copy per location: [N * h * w, 1, T]
    weighted = np.matmul(tiled, m_output)                                       # batched [1, T] x [T, m_rnn]: [N * h * w, 1, m_rnn]
    return attn, weighted[:, 0, :]


def _tensors(v, dtype, names):
    return {k: torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True) for k, a in v.items() if k in names}


def _grads(t):
    return {k: (a.grad.numpy() if a.grad is not None else np.zeros(a.shape)) for k, a in t.items()}


def head_gradients(feat_np, v, indices, seq_len, max_len, dpred_np, dtype=torch.float64, use_attn=True):
    """The gradient of sum(pred * dpred) on every head variable, by autograd -> ({name: array}, pred array)."""
    t = _tensors(v, dtype, HEAD_NAMES if use_attn else TO.HEAD_NAMES)
    pred = head(torch.tensor(np.asarray(feat_np), dtype=dtype), t, indices, seq_len, max_len, use_attn)
    (pred * torch.tensor(np.asarray(dpred_np), dtype=dtype)).sum().backward()
    return _grads(t), pred.detach().numpy()


def train_step_loss(feat_np, v, indices, seq_len, max_len, sketch_u8, target, dtype=torch.float64, use_attn=True):
    """-> (class loss, {name: gradient of the class loss}, pred)."""
    t = _tensors(v, dtype, HEAD_NAMES if use_attn else TO.HEAD_NAMES)
    pred = head(torch.tensor(np.asarray(feat_np), dtype=dtype), t, indices, seq_len, max_len, use_attn)
    loss, _up, _live = TO.class_loss(pred, sketch_u8, target, dtype)
    loss.backward()
    return float(loss.detach()), _grads(t), pred.detach().numpy()


# ------------------------------------------------------------------ RMI_model.py:302-310, 320-330, 367 re-enacted
def reference_variables(w_rnn):
    """What _fully_connected(name='attn_fc', in_dim=w_rnn, out_dim=1) creates under the scope text_sketchyscene:
    [(op name, shape, initialiser: ('uniform', limit) | ('constant', value))].  uniform_unit_scaling_initializer(factor=1.0) draws
    from +-sqrt(3 / input size) * factor, the input size being the product of all dimensions but the last."""
    return [('text_sketchyscene/attn_fc/DW', (w_rnn, 1), ('uniform', float(np.sqrt(3.0 / w_rnn)))),
            ('text_sketchyscene/attn_fc/biases', (1,), ('constant', 0.0))]


def reference_train_rules(op_names):
    """train_op's three comprehensions over the variables' op names -> (tvars, reg_var_list, var_lr_mult)."""
    trained = [n for n in op_names if n[:len('text_sketchyscene')] == 'text_sketchyscene']       # train_fusion_var_only
    regularised = [n for n in trained if 'DW' in n[1:]]              # the substring, found behind the first character
    scale = {n: 2.0 if 'biases' in n[1:] else 1.0 for n in trained}
    return trained, regularised, scale
