"""Training the matcher's fusion head (Instance_Matching/matching_main.py::train, RMI_model.py::train_op with
train_fusion_var_only, utils/loss.py): the backbone stays frozen, the text_sketchyscene/* head -- the visual projection,
the embedding, the word LSTM, the multimodal LSTM and the output projection -- learns.  DESIGN.md section 8.8.

    per iteration  MatchModel.features (frozen backbone) -> head_train (MatchModel.head with keep: every step's state kept)
                   -> ssc_match_loss_grad (summed sigmoid cross entropy of the up-sampled logits over the stroke pixels, its
                   gradient on the 1/8 map) -> backward (ssc_squash_project_bwd, BPTT of both cells on the caption branch's
                   kernels) -> ssc_l2_reg on the two DW -> ssc_adam_tf per tensor (gradient x 2 on the two biases) ->
                   hip.refresh_splits

The trained parameters are the head's entries of MatchModel.flat, in the device layout (LSTM kernels cut by input rows and padded
by gate blocks); the gradient and the two Adam slots are buffers of that layout.  A padded entry has a zero gradient by
construction and Adam leaves a zero with zero moments at zero.

Training the backbone's filters as well: match_backbone_train.py, a subclass of the trainer here.

MatchConfig(use_attn=True): attn_fc/DW and attn_fc/biases are trained too.  MatchModel.head accumulates
the weighted sum of the multimodal outputs; backward sends the projection's gradient into that sum, injects
attn[t] times it into every step of the multimodal cell's BPTT (ssc_dev_scaled_add), takes the weights' gradient as L dots over
the kept outputs (ssc_attn_plane_dots) and goes through the softmax into the two variables and the word cell's incoming gradient
(ssc_attn_scores_bwd).  The bias shifts every logit alike: it is a free parameter, its exact gradient is 0.

Not here: training_ignore_bg = False, the other backbones, fusion_type 'RecurAttn', dropout, summaries, batches, several devices,
a captured step."""
import json
import os
import random

import numpy as np

from . import matching
from .match_backbones import BACKBONES
from .matching import HEAD, pack_head, unpack_head, unpad_gate_columns  # noqa: F401 (the head's packing lives beside pad_lstm)

BETA1, BETA2, EPSILON = 0.9, 0.999, 1e-8
LIVE_MAX_BYTE = 104         # im[..., 0] < 0 with mu_0 = 104.00698793


# ---------------------------------------------------------------------------------------------------------------------------
# host: names, schedule, initialisation, layout
# ---------------------------------------------------------------------------------------------------------------------------
def head_variable_names(config):
    """The trained variables under their checkpoint names, in variable_shapes' order."""
    return [n for n in config.variable_shapes() if n.startswith(HEAD)]


def is_regularized(name):
    """loss.py::l2_regularization_loss: the trained variables whose name contains 'DW'."""
    return 'DW' in name


def grad_scale(name):
    """RMI_model.py::train_op: the gradient of a variable whose name contains 'biases' is doubled before Adam.  Under the
    checkpoint names lstm_cell/bias the LSTM biases are not among them."""
    return 2.0 if 'biases' in name else 1.0


def polynomial_decay(step, start_lr=2.5e-4, end_lr=1e-5, decay_steps=75000, power=0.9):
    """tf.train.polynomial_decay without cycle, in float64."""
    s = min(float(step), float(decay_steps))
    return (float(start_lr) - float(end_lr)) * (1.0 - s / float(decay_steps)) ** float(power) + float(end_lr)


def adam_step_size(lr, t):
    """lr_t of tf.train.AdamOptimizer for its t-th update (t >= 1)."""
    return float(lr) * np.sqrt(1.0 - BETA2 ** t) / (1.0 - BETA1 ** t)


def init_head(config, seed=0):
    """{checkpoint name: float32 array} of a fresh head, the reference's initialisers drawn from numpy.random.RandomState(seed):
    Xavier-uniform for the two DW, uniform +-0.08 for the embedding, Glorot-uniform for the LSTM kernels, zero biases; with
    use_attn uniform_unit_scaling_initializer(factor=1.0), +-sqrt(3 / w_rnn), for attn_fc/DW, drawn last.  (TF's own random
    streams are not reproduced.)"""
    rng = np.random.RandomState(seed)
    out = {}
    shapes = config.variable_shapes()
    for name in head_variable_names(config):
        v = matching.draw_head_weight(rng, name.rsplit('/', 1)[1], shapes[name])
        out[name] = np.ascontiguousarray(np.zeros(shapes[name]) if v is None else v, dtype=np.float32)
    return out


# device name -> the checkpoint variable whose name decides its regulariser and its gradient scale
DEVICE_TO_VARIABLE = {
    'vproj/w': 'visual_feat_projection/DW', 'vproj/b': 'visual_feat_projection/biases', 'embedding': 'embedding',
    'w/Kx': 'wLSTM/lstm_cell/kernel', 'w/Kh': 'wLSTM/lstm_cell/kernel', 'w/b': 'wLSTM/lstm_cell/bias',
    'm/Kv': 'mLSTM/lstm_cell/kernel', 'm/Kw': 'mLSTM/lstm_cell/kernel', 'm/Kl': 'mLSTM/lstm_cell/kernel',
    'm/Ks': 'mLSTM/lstm_cell/kernel', 'm/Kh': 'mLSTM/lstm_cell/kernel', 'm/b': 'mLSTM/lstm_cell/bias',
    'proj/w': 'm_lstm_output_projection/DW', 'proj/b': 'm_lstm_output_projection/biases',
}
HEAD_DEVICE_NAMES = tuple(DEVICE_TO_VARIABLE)
ATTN_DEVICE_TO_VARIABLE = {'attn/w': 'attn_fc/DW', 'attn/b': 'attn_fc/biases'}      # use_attn: behind proj/b


def device_to_variable(config):
    """DEVICE_TO_VARIABLE of a configuration: with use_attn the attention's two tensors behind the others."""
    return dict(DEVICE_TO_VARIABLE, **ATTN_DEVICE_TO_VARIABLE) if config.use_attn else dict(DEVICE_TO_VARIABLE)


def head_device_names(config):
    """HEAD_DEVICE_NAMES of a configuration, in the flat buffer's order."""
    return tuple(device_to_variable(config))


# ---------------------------------------------------------------------------------------------------------------------------
# the order of the training tuples
# ---------------------------------------------------------------------------------------------------------------------------
def training_tuples(scenes):
    """match_eval.read_captions' list -> [(image id, caption, inst_indices)] in the file's order."""
    return [(image_id, caption, list(idx)) for image_id, pairs in scenes for caption, idx in pairs]


class TupleCursor(object):
    """The reference's walk over its tuples: an index list shuffled by ``rng`` every time the cursor wraps to 0, one tuple per
    iteration.  ``state`` / ``restore`` carry the cursor, the shuffled order and the generator over a snapshot."""

    def __init__(self, n, rng):
        if n < 1:
            raise ValueError('no training tuple')
        self.n, self.rng, self.cursor, self.order = int(n), rng, -1, list(range(int(n)))

    def next(self):
        self.cursor = (self.cursor + 1) % self.n
        if self.cursor == 0:
            self.rng.shuffle(self.order)
        return self.order[self.cursor]

    def state(self):
        version, internal, gauss = self.rng.getstate()
        return {'cursor': self.cursor, 'order': list(self.order), 'rng': [version, list(internal), gauss]}

    def restore(self, state):
        if len(state['order']) != self.n:
            raise ValueError('the saved order holds %d tuples, the caption file %d' % (len(state['order']), self.n))
        self.cursor, self.order = int(state['cursor']), [int(i) for i in state['order']]
        version, internal, gauss = state['rng']
        self.rng.setstate((version, tuple(internal), gauss))


def caption_lut(labels_of_caption):
    """The labels of a caption's instances (match_eval.caption_labels) -> uint8 [256]: 1 at every label of the target."""
    lut = np.zeros(256, dtype=np.uint8)
    lut[np.asarray(sorted(set(int(g) for g in labels_of_caption)), dtype=np.int64)] = 1
    return lut


# ---------------------------------------------------------------------------------------------------------------------------
# a trained stretch of MatchModel.flat: its buffers, its update, its Adam slots in a snapshot
# ---------------------------------------------------------------------------------------------------------------------------
def trained_stretch(model, names, lo, hi):
    """flat[lo:hi] holds the tensors ``names`` (layout names, in the layout's order) -> (the stretch, its gradient buffer and its
    two Adam slot buffers, {name: (offset in the stretch, real size, size up to the next tensor of the layout, shape)}, the
    three buffers' views by name)."""
    import torch
    lay, order = model._layout, list(model._layout)
    bufs = [torch.zeros(hi - lo, dtype=torch.float32, device=model.device) for _ in range(3)]
    spans = {}
    for name in names:
        o, shape = lay[name]
        spans[name] = (o - lo, int(np.prod(shape)), lay[order[order.index(name) + 1]][0] - o, shape)
    views = [{n: buf[o:o + size].view(shape) for n, (o, size, _p, shape) in spans.items()} for buf in bufs]
    return model.flat[lo:hi], bufs, spans, views


def apply_adam(params, grad, adam_m, adam_v, spans, variable_of, lr_t, weight_decay):
    """One update of a stretch: the regulariser's gradient on the real entries of every span whose variable is_regularized, TF's
    Adam on every span (padding included: a zero with zero moments stays zero) with the gradient times its variable's
    grad_scale, then the bf16 planes of the changed filters."""
    from . import hip
    for name, (o, size, _padded, _shape) in spans.items():
        if is_regularized(variable_of[name]) and weight_decay != 0.0:
            hip.call('ssc_l2_reg', params[o:o + size], size, weight_decay, None, grad[o:o + size])
    for name, (o, _size, padded, _shape) in spans.items():
        hip.call('ssc_adam_tf', params[o:o + padded], grad[o:o + padded], adam_m[o:o + padded], adam_v[o:o + padded], padded, lr_t,
                 None, BETA1, BETA2, EPSILON, grad_scale(variable_of[name]))
    hip.refresh_splits(params)


def slots_to_snapshot(out, m, v, to_checkpoint):
    """The two Adam slots of a stretch into ``out`` as <name>/Adam and <name>/Adam_1; to_checkpoint: views by layout name ->
    {checkpoint name: array}."""
    for suffix, views in (('/Adam', m), ('/Adam_1', v)):
        for name, a in to_checkpoint(views).items():
            out[name + suffix] = a


def slots_from_snapshot(tensors, m, v, names, from_checkpoint, hint):
    """The way back: the slots of the checkpoint variables ``names`` out of a snapshot's tensors; from_checkpoint: {checkpoint
    name: array} -> {layout name: array}.  ValueError with ``hint`` for a snapshot without them."""
    import torch
    for suffix, views in (('/Adam', m), ('/Adam_1', v)):
        host = {}
        for name in names:
            if name + suffix not in tensors:
                raise ValueError('the snapshot has no %s: %s' % (name + suffix, hint))
            host[name] = tensors[name + suffix]
        for n, a in from_checkpoint(host).items():
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.shape != tuple(views[n].shape):
                raise ValueError('%s is %s, the model needs %s' % (n + suffix, a.shape, tuple(views[n].shape)))
            views[n].copy_(torch.from_numpy(a))


# ---------------------------------------------------------------------------------------------------------------------------
# the trainer on the device
# ---------------------------------------------------------------------------------------------------------------------------
class MatchTrainer(object):
    """Wraps a loaded MatchModel.  ``g``, ``m`` and ``v`` are views into the gradient buffer and the two Adam slot buffers by the
    device names of the head."""

    def __init__(self, model, weight_decay=5e-4):
        import torch
        if not model.loaded:
            raise RuntimeError('the matcher has no weights: load_tf_checkpoint, load_dict or init_random first')
        self.model, self.cfg = model, model.cfg
        self.weight_decay = float(weight_decay)
        lay = model._layout
        self.dev_to_var = device_to_variable(self.cfg)
        self.names = names = head_device_names(self.cfg)
        assert [n for n in lay if n in self.dev_to_var] == list(names), list(lay)
        self.lo, self.hi = lay[names[0]][0], lay['spatial'][0]
        # the head is one stretch of the flat buffer: every trained tensor in it, nothing else
        inside = [n for n, (o, _s) in lay.items() if self.lo <= o < self.hi]
        assert inside == list(names), inside
        self.params, (self.grad, self.adam_m, self.adam_v), self.spans, (self.g, self.m, self.v) = \
            trained_stretch(model, names, self.lo, self.hi)
        self.step_count = 0
        self._loss = torch.zeros(2, dtype=torch.float64, device=model.device)
        self._live = torch.zeros(2, dtype=torch.int64, device=model.device)
        self._loss_host, self._loss_event = None, [None, None]
        self._ctx = None

    # ------------------------------------------------------------------ forward
    def head_train(self, feat, tok, seq_len):
        """MatchModel.head with the cell state, the output and the activated gates of every step of both cells kept for
        ``backward``: the same pass, so ``pred`` has its bits."""
        ctx = {}
        pred = self.model.head(feat, tok, seq_len, keep=ctx)
        self._ctx = ctx
        return pred

    # ------------------------------------------------------------------ backward
    def backward(self, dpred, dfeat=None):
        """dpred float [h,w]: the gradient on ``head_train``'s pred.  Fills the gradient of every trained tensor (device layout).
        dfeat float [1,h,w,feat_channels]: receives the gradient on ``head_train``'s feat (match_backbone_train.py); without it
        nothing goes into the backbone."""
        import torch
        from . import hip
        from .hip import View
        mdl, c, d, g, x = self.model, self.cfg, self.model.d, self.g, self._ctx
        if x is None:
            raise RuntimeError('backward without a head_train before it')
        buf = mdl._buf
        L, R, cw, cm = x['L'], x['R'], mdl.cw, mdl.cm
        G4 = 4 * cm
        one = mdl.one
        ca, ha, acts_m = x['ca'], x['ha'], x['acts_m']
        ws = hip.workspace()
        # 1. the projection and the squash
        dh, dh2 = buf('b_dh0', (R, cm)), buf('b_dh1', (R, cm))
        dc, dc2 = buf('b_dc0', (R, cm)), buf('b_dc1', (R, cm))
        attn, dacc, dattn = x['attn'], None, None
        if attn is None:
            hip.squash_project_bwd(ha[L], d['proj/w'], dpred.reshape(-1), C=c.m_rnn, dh=dh, dw=g['proj/w'], db=g['proj/b'], ws=ws)
        else:       # the projection read the weighted sum: its gradient reaches every step's output through that step's weight,
            #         and the weights through the L dots <dacc, m_out[t]> (taken now: ws is free again before the next user)
            dacc = buf('b_dacc', (R, cm))
            hip.squash_project_bwd(x['acc'], d['proj/w'], dpred.reshape(-1), C=c.m_rnn, dh=dacc, dw=g['proj/w'], db=g['proj/b'], ws=ws)
            dattn = hip.attn_plane_dots(dacc, ha[1:], L, out=buf('b_dattn', (c.max_len,)), ws=ws)
        # 2. the multimodal cell back through its steps: the gate gradients of every step are kept, their sum is the gradient of
        #    the step-invariant share of the gates
        dg_all, dgs = buf('b_dg_all', (c.max_len, R, G4)), buf('b_dgs', (R, G4))
        hip.fill(dc, 0.0)
        hip.fill(dgs, 0.0)
        for t in range(L - 1, -1, -1):
            if attn is not None:    # dh = (what step t + 1 sent back) + attn[t] * dacc
                hip.dev_scaled_add(dh, dacc, attn, t, overwrite=t == L - 1)
            hip.call('ssc_lstm_pointwise_bwd', dh, dc, acts_m[t], ca[t], ca[t + 1], one, R, R, cm, dg_all[t], dc2, dh2, dgs)
            if t > 0:       # h_0 = 0: nothing upstream of it
                hip.matmul_nt(dg_all[t], d['m/Kh'], dh2, accumulate=True)
            dh, dh2 = dh2, dh
            dc, dc2 = dc2, dc
        # 3. its filter gradients, batched over the steps
        if L > 1:
            hip.matmul_tn(ha[1:L].reshape((L - 1) * R, cm), dg_all[1:L].reshape((L - 1) * R, G4), g['m/Kh'])
        else:
            hip.fill(g['m/Kh'], 0.0)
        hip.matmul_tn(x['vis'], dgs, g['m/Kv'])
        hip.matmul_tn(d['spatial'], dgs, g['m/Ks'])
        # 4. the words' share of the gates: one row per step
        dr = buf('b_dr', (c.max_len, G4))
        hip.call('ssc_group_rowsum', dg_all, G4, L, R, G4, dr, 0)
        hip.call('ssc_group_rowsum', dr, G4, 1, L, G4, g['m/b'], 0)
        emb, lang = x['emb'], x['lang']
        hip.matmul_tn(emb[:L], dr[:L], g['m/Kw'])
        hip.matmul_tn(lang[:L], dr[:L], g['m/Kl'])
        demb, dlang = buf('b_demb', (c.max_len, c.w_emb)), buf('b_dlang', (c.max_len, cw))
        hip.matmul_nt(dr[:L], d['m/Kw'], demb[:L])
        hip.matmul_nt(dr[:L], d['m/Kl'], dlang[:L])
        dhw = buf('b_dhw', (c.max_len, cw))
        hip.call('ssc_row_l2norm_bwd', lang, x['lang_ss'], dlang, L, cw, dhw, 0)
        if attn is not None:    # through the softmax: the two variables, and dlogit[t] * w onto the word outputs' gradient
            hip.attn_scores_bwd(attn, dattn, x['hs'][1:], d['attn/w'], c.w_rnn, L, dhs=dhw, dw=g['attn/w'], db=g['attn/b'],
                                dlogit=buf('b_dlogit', (c.max_len,)))
        # 5. the word cell back through its steps, then the embedding
        cs, hs, acts_w = x['cs'], x['hs'], x['acts_w']
        dew = buf('b_dew', (c.max_len, 4 * cw))
        wh, wh2, wc, wc2 = (buf('b_w%d' % k, (1, cw)) for k in range(4))
        hip.fill(wh, 0.0)
        hip.fill(wc, 0.0)
        for t in range(L - 1, -1, -1):
            hip.call('ssc_axpy', wh, dhw[t:t + 1], 1.0, cw)
            hip.call('ssc_lstm_pointwise_bwd', wh, wc, acts_w[t], cs[t:t + 1], cs[t + 1:t + 2], one, 1, 1, cw, dew[t:t + 1], wc2,
                     wh2, None)
            if t > 0:
                hip.matmul_nt(dew[t:t + 1], d['w/Kh'], wh2, accumulate=True)
            wh, wh2 = wh2, wh
            wc, wc2 = wc2, wc
        if L > 1:
            hip.matmul_tn(hs[1:L], dew[1:L], g['w/Kh'])
        else:
            hip.fill(g['w/Kh'], 0.0)
        hip.matmul_tn(emb[:L], dew[:L], g['w/Kx'])
        hip.matmul_nt(dew[:L], d['w/Kx'], demb[:L], accumulate=True)
        hip.call('ssc_group_rowsum', dew, 4 * cw, 1, L, 4 * cw, g['w/b'], 0)
        hip.fill(g['embedding'], 0.0)
        hip.call('ssc_embedding_scatter_add', g['embedding'], c.vocab_size, x['tok'], L, c.w_emb, demb)
        # 6. the visual branch, down to the projection's filter
        dvis, dvp = buf('b_dvis', (R, c.v_emb)), buf('b_dvp', (R, c.v_emb))
        hip.matmul_nt(dgs, d['m/Kv'], dvis)
        hip.call('ssc_row_l2norm_bwd', x['vis'], x['vis_ss'], dvis, R, c.v_emb, dvp, 0)
        hip.conv_wgrad(View(x['feat']), View(dvp.view(1, x['fh'], x['fw'], c.v_emb)), g['vproj/w'], 1, 0)
        hip.join_wgrad()
        hip.call('ssc_group_rowsum', dvp, c.v_emb, 1, R, c.v_emb, g['vproj/b'], 0)
        if dfeat is not None:       # d feat = dvp . DW^T
            hip.matmul_nt(dvp, d['vproj/w'].view(c.feat_channels, c.v_emb), dfeat.view(R, c.feat_channels))

    # ------------------------------------------------------------------ loss, optimiser
    def loss_and_grad(self, pred, sketch_d, labels_d, lut_d, slot=0):
        """-> dpred float [h,w]; the class loss is added into the double of ``slot`` (zeroed here), the live count stored."""
        from . import hip
        fh, fw = pred.shape
        self._loss[slot:slot + 1].zero_()
        dpred = self.model._buf('t_dpred', (fh, fw))
        hip.match_loss_grad(pred, sketch_d, labels_d, lut_d, self._loss[slot:slot + 1], live=self._live[slot:slot + 1], dpred=dpred,
                            ws=hip.workspace())
        return dpred

    def apply(self, lr):
        """The regulariser's gradient on the two DW, then TF's Adam on every trained tensor with the gradient of the two biases
        doubled, then the bf16 planes of the changed filters."""
        self.step_count += 1
        apply_adam(self.params, self.grad, self.adam_m, self.adam_v, self.spans, self.dev_to_var, adam_step_size(lr, self.step_count),
                   self.weight_decay)

    def upload_scene(self, labels_u8):
        """The scene's label map uint8 [S,S] into its device buffer (once per scene)."""
        import torch
        c = self.cfg
        labels = np.ascontiguousarray(labels_u8, dtype=np.uint8)
        if labels.shape != (c.size, c.size):
            raise ValueError('the label map is %s, the matcher trains on [%d, %d]' % (labels.shape, c.size, c.size))
        d = self.model._buf('t_labels', (c.size, c.size), torch.uint8)
        d.copy_(torch.from_numpy(labels))
        return d

    def _resident(self, t, shape, dtype, what):
        if t.device.type != self.model.device.type or t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
            raise ValueError('%s is %s %s on %s, the step reads a contiguous %s %s on %s'
                             % (what, t.dtype, tuple(t.shape), t.device, dtype, tuple(shape), self.model.device))
        return t

    def step(self, scene, lut, tok, seq_len, lr):
        """scene: {'sketch': uint8 [S,S,3], 'labels': uint8 [S,S]} (host arrays, or a dict ``upload_scene`` has been applied to:
        'labels_d'), or its device-resident form (match_cache.MatchSceneCache.entry): {'sketch_d': uint8 [S,S,3], 'labels_d':
        uint8 [S,S]} on the device, the loss reads them where they are, and with 'feat_d' float [1,S/8,S/8,feat_channels] -- what
        MatchModel.features gives for that sketch -- the backbone does not run; lut uint8 [256]; tok the sentence's max_len
        indices; seq_len its real length; lr the step's learning rate.
        One iteration.  -> the class loss of the PREVIOUS step (None at the first): the value is read one step late, the step
        itself never waits for the device.  ``last_loss`` reads the current one on demand."""
        import torch
        c, mdl = self.cfg, self.model
        tok, seq_len = mdl.check_sentence(tok, seq_len)
        lut = np.ascontiguousarray(lut, dtype=np.uint8).reshape(-1)
        if lut.shape[0] != 256:
            raise ValueError('the lut holds %d bytes, not 256' % lut.shape[0])
        prev = self._take_loss((self.step_count + 1) & 1)
        slot = self.step_count & 1
        if 'sketch_d' in scene:
            sketch_d, labels_d = self._resident(scene['sketch_d'], (c.size, c.size, 3), torch.uint8, 'sketch_d'), \
                self._resident(scene['labels_d'], (c.size, c.size), torch.uint8, 'labels_d')
            if 'feat_d' in scene:       # the frozen backbone's output is given: neither the preprocessing nor the backbone runs
                feat = self._resident(scene['feat_d'], (1, c.feat, c.feat, c.feat_channels), torch.float32, 'feat_d')
            else:
                feat = self._features(sketch_d)
        else:
            feat = self._features(scene['sketch'])
            sketch_d = mdl._buf('sketch', (c.size, c.size, 3), torch.uint8)
            labels_d = scene['labels_d'] if 'labels_d' in scene else self.upload_scene(scene['labels'])
        tok_d = mdl.put_sentence(tok)
        lut_d = mdl._buf('t_lut', (256,), torch.uint8)
        lut_d.copy_(torch.from_numpy(lut))
        pred = self.head_train(feat, tok_d, seq_len)
        dpred = self.loss_and_grad(pred, sketch_d, labels_d, lut_d, slot)
        if self._loss_host is None:
            self._loss_host = torch.zeros(2, dtype=torch.float64).pin_memory()
        self._loss_host[slot:slot + 1].copy_(self._loss[slot:slot + 1], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._loss_event[slot] = ev
        self.backward(dpred)
        self.apply(lr)
        return prev

    def _features(self, sketch):
        """The visual feature of a sketch for ``step``: the frozen backbone's (match_backbone_train.py keeps what its backward
        needs instead)."""
        return self.model.features(sketch)[0]

    def _take_loss(self, slot):
        ev = self._loss_event[slot]
        if ev is None:
            return None
        ev.synchronize()
        return float(self._loss_host[slot])

    def last_loss(self):
        """The class loss of the latest step (waits for it)."""
        return self._take_loss((self.step_count + 1) & 1)

    # ------------------------------------------------------------------ weights in and out
    def _export(self, views):
        return unpack_head(self.cfg, {n: views[n].detach().cpu().numpy() for n in self.names})

    def export_variables(self):
        """{checkpoint name: array}: the head out of the device layout, and the backbone's arrays as they were loaded.
        MatchModel.load_dict of it reproduces the device buffer bit for bit."""
        out = {k: v for k, v in self.model.host.items() if not k.startswith(HEAD)}
        out.update(self._export(self.model.d))
        return out

    def export_gradients(self):
        return self._export(self.g)

    def snapshot_tensors(self):
        """What a snapshot holds: every variable, the Adam slots of the trained ones as <name>/Adam and <name>/Adam_1,
        beta1_power, beta2_power and the step as Variable."""
        out = self.export_variables()
        slots_to_snapshot(out, self.m, self.v, self._export)
        out['beta1_power'] = np.float32(BETA1 ** (self.step_count + 1))
        out['beta2_power'] = np.float32(BETA2 ** (self.step_count + 1))
        out['Variable'] = np.int32(self.step_count)
        return out

    def load_slots(self, tensors, step):
        """The Adam slots and the step out of a snapshot's tensors."""
        slots_from_snapshot(tensors, self.m, self.v, head_variable_names(self.cfg), lambda host: pack_head(self.cfg, host),
                            'it was not written by training')
        self.step_count = int(step)


def model_name(backbone='deeplab'):
    """The reference's weights_name + '_' + model_name: deeplab_RMI, segnet_RMI."""
    return BACKBONES[backbone].model_name


def snapshot_prefix(snapshot_root, iteration, backbone='deeplab'):
    return os.path.join(snapshot_root, '%s_iter_%d.tfmodel' % (model_name(backbone), iteration))


def write_snapshot(trainer, snapshot_root, iteration, cursor):
    """<snapshot_root>/<deeplab|segnet>_RMI_iter_<n>.tfmodel.{index, data-00000-of-00001}, the ``checkpoint`` file that names it
    and <prefix>.train_state.json with the cursor, the shuffled order and the generator's state.  -> the prefix."""
    from . import tf_checkpoint
    os.makedirs(snapshot_root, exist_ok=True)
    prefix = snapshot_prefix(snapshot_root, iteration, trainer.cfg.backbone)
    tf_checkpoint.write_checkpoint(prefix, trainer.snapshot_tensors())
    with open(prefix + '.train_state.json', 'w') as f:
        json.dump(dict(cursor.state(), iteration=int(iteration)), f)
    base = os.path.basename(prefix)
    with open(os.path.join(snapshot_root, 'checkpoint'), 'w') as f:
        f.write('model_checkpoint_path: "%s"\nall_model_checkpoint_paths: "%s"\n' % (base, base))
    return prefix


def snapshot_iteration(prefix):
    """The iteration in a snapshot's name, as the reference reads it: between the last '_' and the last '.'."""
    try:
        return int(prefix[prefix.rfind('_') + 1:prefix.rfind('.')])
    except ValueError:
        raise ValueError('%r: no iteration in the snapshot name' % prefix)
