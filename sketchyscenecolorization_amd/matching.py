"""The instance matcher of the scene pipeline, batch 1 (Pipeline_utils/fg_matching_utils.py::build_instance_matching): RMI_model.py
(fusion_type 'RMI') on one of its backbones, then get_pred_instance_mask's choice of the instances the prediction covers.  This
module holds the host side (text, padding, MatchConfig), the fusion head and the whole pass, for inference and -- with ``keep`` --
as the forward pass of training; everything that depends on which backbone runs is in match_backbones.py.  DESIGN.md section 8.6.
MatchConfig(use_attn=True): the model class's word attention (RMI_model.py:202-217) -- a softmax over the word LSTM's outputs
weighs the multimodal LSTM's outputs of every word, their sum feeds the projection; DESIGN.md section 8.11.

    sketch uint8 [S,S,3] --ssc_match_preprocess_u8--> x [1,S,S,4], stroke [S,S]
    backbone: MatchModel.backbone -> MatchConfig.net.forward, the pass of a class of match_backbones.py on this model's buffers
              and weights -> the visual feature [1,S/8,S/8,feat_channels].  MatchConfig(backbone='deeplab'): the DeepLab-ResNet of
              deeplab_model.py, frozen norms (DeepLabBackbone); 'segnet': SegNet of segnet_model.py, the norms of the one image
              (SegNetBackbone)
    head:     1x1 projection + l2 norm, word LSTM, multimodal LSTM per location (hip.lstm_step_fwd on gate blocks padded to a
              multiple of 32), ssc_squash_project, ssc_match_finish -> up [S,S], predicts [S,S]
              use_attn: ssc_attn_scores_fwd behind the word LSTM, ssc_dev_scaled_add behind every multimodal step, and
              ssc_squash_project on the weighted sum instead of the last state
    choice:   ssc_instance_occupancy -> int64 counts; the quotient and the comparison with 0.5 in float64 on the host

``features`` and ``predict`` are the pass in two halves -- the backbone once per scene, the head once per caption -- for the
evaluation on a split (match_eval.py).

``head``, ``backbone`` and ``features`` are also the forward pass of training: with ``keep`` they leave what a backward pass reads
in buffers of its own (match_train.py, match_backbone_train.py; DESIGN.md sections 8.8 and 8.10).

Not here: the backward pass and the optimiser (match_train.py), the backbones fcn_8s and deeplab_v3plus,
SegNet's backward, fusion_type 'RecurAttn', post_processing_mask_with_segmentation."""
import os
import re

import numpy as np

from .match_backbones import BACKBONES, NORM_PARTS, fold_norm  # noqa: F401 (folding a frozen norm stays part of the host interface)

OCCUPIED_THRESH = 0.5
UNK, PAD = '<unk>', '<pad>'
_SPLIT = re.compile(r'(\W+)')
ATTN_MAX_LEN = 64           # hip.ATTN_MAX_T: the words the attention kernels hold
HEAD = 'text_sketchyscene/'          # the scope of the fusion head's variables
ATTN_VARIABLES = (HEAD + 'attn_fc/DW', HEAD + 'attn_fc/biases')


# ---------------------------------------------------------------------------------------------------------------------------
# host: text, spatial table, padding
# ---------------------------------------------------------------------------------------------------------------------------
def load_vocab(path):
    """One word per line -> {word: line number} (load_vocab_dict_from_file)."""
    with open(path) as f:
        words = [w.strip() for w in f.readlines()]
    return {w: n for n, w in enumerate(words)}


def sentence_tokens(text):
    """The words the matcher reads: split on (\\W+), lower-cased, without blanks and '-', without a final '.'."""
    words = [w.lower() for w in _SPLIT.split(text.strip()) if len(w.strip()) > 0 and w != '-']
    if words and words[-1] == '.':
        words = words[:-1]
    return words


def preprocess_sentence(text, vocab, T=15):
    """-> (T vocabulary indices, the number of real ones): unknown words become <unk>, a long sentence is cut at T, a short one
    padded on the right with <pad>.  ValueError for a sentence without a token."""
    words = sentence_tokens(text)
    if not words:
        raise ValueError('%r holds no word for the matcher' % (text,))
    idx = [vocab[w] if w in vocab else vocab[UNK] for w in words][:T]
    n = len(idx)
    return idx + [vocab[PAD]] * (T - n), n


def spatial_features(h, w):
    """generate_spatial_batch for one image: float32 [h,w,8] = (xmin, ymin, xmax, ymax, xctr, yctr, 1/w, 1/h), in [-1, 1]."""
    out = np.zeros((h, w, 8), dtype=np.float32)
    for y in range(h):
        for x in range(w):
            xmin, xmax = x / w * 2 - 1, (x + 1) / w * 2 - 1
            ymin, ymax = y / h * 2 - 1, (y + 1) / h * 2 - 1
            out[y, x, :] = [xmin, ymin, xmax, ymax, (xmin + xmax) / 2, (ymin + ymax) / 2, 1 / w, 1 / h]
    return out


def pad32(c):
    return -(-c // 32) * 32


def pad_gate_columns(k, c, cp):
    """[..., 4c] (gate blocks i, j, f, o) -> [..., 4cp]: every block laid out at the padded width, zeros between."""
    k = np.asarray(k)
    out = np.zeros(k.shape[:-1] + (4 * cp,), dtype=k.dtype)
    for g in range(4):
        out[..., g * cp:g * cp + c] = k[..., g * c:(g + 1) * c]
    return out


def pad_rows(k, rows):
    k = np.asarray(k)
    out = np.zeros((rows,) + k.shape[1:], dtype=k.dtype)
    out[:k.shape[0]] = k
    return out


def pad_lstm(kernel, bias, n_in, c):
    """LSTMCell's kernel [n_in + c, 4c] and bias [4c] -> (Kx [n_in, 4cp], Kh [cp, 4cp], bias [4cp]), cp = c rounded up to a
    multiple of 32.  The padded units see zero gates: c' = c*sigmoid(1) + sigmoid(0)*tanh(0) stays 0 and h' = tanh(0)*sigmoid(0)
    stays 0, and their zero rows of Kh give nothing to the real units."""
    kernel, bias = np.asarray(kernel), np.asarray(bias)
    cp = pad32(c)
    assert kernel.shape == (n_in + c, 4 * c) and bias.shape == (4 * c,), (kernel.shape, bias.shape, n_in, c)
    return (pad_gate_columns(kernel[:n_in], c, cp), pad_rows(pad_gate_columns(kernel[n_in:], c, cp), cp),
            pad_gate_columns(bias, c, cp))


def unpad_gate_columns(k, c, cp):
    """The inverse of pad_gate_columns: [..., 4cp] -> [..., 4c]."""
    k = np.asarray(k)
    return np.concatenate([k[..., g * cp:g * cp + c] for g in range(4)], axis=-1)


def pack_head(config, host):
    """{checkpoint name: array} of the head -> {device name: float32 array}, as the kernels read them: the LSTM kernels cut by
    input rows and padded by gate blocks, the two projections' vectors padded."""
    c, h = config, HEAD
    cw, cm = pad32(c.w_rnn), pad32(c.m_rnn)
    dev = {'vproj/w': host[h + 'visual_feat_projection/DW'], 'vproj/b': host[h + 'visual_feat_projection/biases'],
           'embedding': host[h + 'embedding']}
    dev['w/Kx'], dev['w/Kh'], dev['w/b'] = pad_lstm(host[h + 'wLSTM/lstm_cell/kernel'], host[h + 'wLSTM/lstm_cell/bias'], c.w_emb, c.w_rnn)
    kx, dev['m/Kh'], dev['m/b'] = pad_lstm(host[h + 'mLSTM/lstm_cell/kernel'], host[h + 'mLSTM/lstm_cell/bias'],
                                           c.v_emb + c.w_emb + c.w_rnn + 8, c.m_rnn)
    o = c.v_emb + c.w_emb
    dev['m/Kv'], dev['m/Kw'] = kx[:c.v_emb], kx[c.v_emb:o]
    dev['m/Kl'], dev['m/Ks'] = pad_rows(kx[o:o + c.w_rnn], cw), kx[o + c.w_rnn:]
    dev['proj/w'] = pad_rows(np.asarray(host[h + 'm_lstm_output_projection/DW']).reshape(-1), cm)
    dev['proj/b'] = host[h + 'm_lstm_output_projection/biases']
    if c.use_attn:
        dev['attn/w'] = pad_rows(np.asarray(host[h + 'attn_fc/DW']).reshape(-1), cw)
        dev['attn/b'] = host[h + 'attn_fc/biases']
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in dev.items()}


def unpack_head(config, dev):
    """The inverse of ``pack_head``: pad_lstm, pad_rows and the cut of the multimodal kernel's rows undone."""
    c, h = config, HEAD
    cw, cm = pad32(c.w_rnn), pad32(c.m_rnn)
    d = {k: np.asarray(v, dtype=np.float32) for k, v in dev.items()}
    out = {h + 'visual_feat_projection/DW': d['vproj/w'].reshape(1, 1, c.feat_channels, c.v_emb),
           h + 'visual_feat_projection/biases': d['vproj/b'].reshape(c.v_emb),
           h + 'embedding': d['embedding'].reshape(c.vocab_size, c.w_emb)}
    out[h + 'wLSTM/lstm_cell/kernel'] = np.concatenate(
        [unpad_gate_columns(d['w/Kx'], c.w_rnn, cw), unpad_gate_columns(d['w/Kh'][:c.w_rnn], c.w_rnn, cw)], axis=0)
    out[h + 'wLSTM/lstm_cell/bias'] = unpad_gate_columns(d['w/b'], c.w_rnn, cw)
    out[h + 'mLSTM/lstm_cell/kernel'] = np.concatenate(
        [unpad_gate_columns(k, c.m_rnn, cm) for k in (d['m/Kv'], d['m/Kw'], d['m/Kl'][:c.w_rnn], d['m/Ks'], d['m/Kh'][:c.m_rnn])], axis=0)
    out[h + 'mLSTM/lstm_cell/bias'] = unpad_gate_columns(d['m/b'], c.m_rnn, cm)
    out[h + 'm_lstm_output_projection/DW'] = d['proj/w'][:c.m_rnn].reshape(1, 1, c.m_rnn, 1)
    out[h + 'm_lstm_output_projection/biases'] = d['proj/b'].reshape(1)
    if c.use_attn:
        out[h + 'attn_fc/DW'] = d['attn/w'][:c.w_rnn].reshape(c.w_rnn, 1)
        out[h + 'attn_fc/biases'] = d['attn/b'].reshape(1)
    return {k: np.array(v, dtype=np.float32, order='C', copy=True) for k, v in out.items()}


class MatchConfig(object):
    """The sizes of the matcher.  The defaults are the released model; the tests run small ones through the same code.
    backbone: a name of match_backbones.BACKBONES; size, units and filters (None: the released widths) are that backbone's, whose
    object is ``net``."""

    def __init__(self, size=768, units=(3, 4, 23, 3), filters=None, v_emb=1000, w_emb=1000, w_rnn=1000,
                 m_rnn=500, vocab_size=76, max_len=15, use_attn=False, backbone='deeplab'):
        if use_attn not in (False, True, 0, 1):
            raise ValueError('use_attn %r: False or True' % (use_attn,))
        if backbone not in BACKBONES:
            raise ValueError("backbone %r: %s; the other backbones are not built" % (backbone, ' or '.join(map(repr, BACKBONES))))
        self.use_attn, self.backbone = bool(use_attn), backbone
        self.v_emb, self.w_emb, self.w_rnn, self.m_rnn = int(v_emb), int(w_emb), int(w_rnn), int(m_rnn)
        self.vocab_size, self.max_len = int(vocab_size), int(max_len)
        self.net = net = BACKBONES[backbone](size, units, filters)      # the backbone object: everything that depends on which one
        self.size, self.units, self.filters = net.size, net.units, net.filters
        self.feat_channels = net.feat_channels      # the channels of the visual feature map
        net.check_widths([('v_emb', self.v_emb), ('w_emb', self.w_emb), ('w_rnn', self.w_rnn), ('m_rnn', self.m_rnn)])
        if self.vocab_size < 2 or self.max_len < 1:
            raise ValueError('vocab_size %d, max_len %d' % (self.vocab_size, self.max_len))
        if self.use_attn and self.max_len > ATTN_MAX_LEN:
            raise ValueError('max_len %d with use_attn: the attention kernels hold %d words' % (self.max_len, ATTN_MAX_LEN))

    @property
    def feat(self):
        return self.size // 8

    def variable_shapes(self):
        """{checkpoint name: shape} of everything inference reads: the backbone's variables (and what rides along unread with
        them), then the head's."""
        s = self.net.variable_shapes()
        h = HEAD
        s[h + 'visual_feat_projection/DW'] = (1, 1, self.feat_channels, self.v_emb)
        s[h + 'visual_feat_projection/biases'] = (self.v_emb,)
        s[h + 'embedding'] = (self.vocab_size, self.w_emb)
        s[h + 'wLSTM/lstm_cell/kernel'] = (self.w_emb + self.w_rnn, 4 * self.w_rnn)
        s[h + 'wLSTM/lstm_cell/bias'] = (4 * self.w_rnn,)
        s[h + 'mLSTM/lstm_cell/kernel'] = (self.v_emb + self.w_emb + self.w_rnn + 8 + self.m_rnn, 4 * self.m_rnn)
        s[h + 'mLSTM/lstm_cell/bias'] = (4 * self.m_rnn,)
        s[h + 'm_lstm_output_projection/DW'] = (1, 1, self.m_rnn, 1)
        s[h + 'm_lstm_output_projection/biases'] = (1,)
        if self.use_attn:
            s[h + 'attn_fc/DW'] = (self.w_rnn, 1)
            s[h + 'attn_fc/biases'] = (1,)
        return s


def check_attention_variables(names, use_attn):
    """names: the variable names of a checkpoint (any container).  ValueError when the attention's variables are missing with
    use_attn, or there without it: a head trained to be read through its attention gives nothing meaningful through its last
    state.  A checkpoint without a head at all (a backbone's) passes with the flag off."""
    for name in ATTN_VARIABLES:
        if use_attn and name not in names:
            raise ValueError('the checkpoint has no variable %s: it was not trained with use_attn (--use_attn 1); read it with '
                             'use_attn off (--use_attn 0)' % name)
        if not use_attn and name in names:
            raise ValueError('the checkpoint holds %s: its head was trained with use_attn (--use_attn 1) and is read through its '
                             'attention; set use_attn (--use_attn 1)' % name)


OLD_CELL_NAMES = {'/lstm_cell/kernel': '/lstm_cell/weights', '/lstm_cell/bias': '/lstm_cell/biases'}


def draw_head_weight(rng, leaf, shape):
    """The reference's initialiser of one of the head's weights, drawn from ``rng``: Xavier-uniform for a 1x1 filter DW,
    uniform_unit_scaling_initializer(factor=1.0) for attn_fc's 2-d DW, Glorot-uniform for an LSTM kernel, uniform +-0.08 for the
    embedding.  -> float64, or None for a leaf that is none of them (a bias)."""
    if leaf == 'DW' and len(shape) == 2:
        return rng.uniform(-1, 1, shape) * np.sqrt(3.0 / shape[0])
    if leaf == 'DW':
        return rng.uniform(-1, 1, shape) * np.sqrt(6.0 / (shape[2] + shape[3]))
    if leaf == 'kernel':
        return rng.uniform(-1, 1, shape) * np.sqrt(6.0 / (shape[0] + shape[1]))
    if leaf == 'embedding':
        return rng.uniform(-0.08, 0.08, shape)
    return None


def random_variables(config, seed=0):
    """Float32 variables under the checkpoint names: the reference's initialisers for the weights, and norms that are not the
    identity (so that a wrong fold shows)."""
    rng = np.random.RandomState(seed)
    out = {}
    for name, shape in config.variable_shapes().items():
        leaf = name.rsplit('/', 1)[1]
        n = int(np.prod(shape))
        if leaf == 'DW' and not name.startswith(HEAD):           # a backbone's filter
            v = rng.randn(*shape) * np.sqrt(2.0 / (shape[0] * shape[1] * shape[3]))
        elif leaf in ('DW', 'kernel', 'embedding'):
            v = draw_head_weight(rng, leaf, shape)
        elif leaf in ('gamma', 'variance', 'moving_variance'):
            v = rng.uniform(0.5, 1.5, shape)
        elif leaf == 'factor':
            v = rng.uniform(0.8, 1.25, shape)
        elif leaf in ('beta', 'mean', 'bias', 'biases', 'moving_mean'):
            v = rng.randn(n).reshape(shape) * 0.1
        else:
            raise AssertionError(name)
        out[name] = np.ascontiguousarray(v, dtype=np.float32)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the model on the device
# ---------------------------------------------------------------------------------------------------------------------------
class MatchModel(object):
    """Weights in one flat device buffer (registered with hip, so that the bf16 planes of its filters are kept), every
    intermediate buffer allocated at first use and kept: a forward pass allocates nothing."""

    def __init__(self, config=None, device='cuda'):
        import torch
        from . import hip
        self.cfg = config if config is not None else MatchConfig()
        self.device = torch.device(device)
        c = self.cfg
        self.cw, self.cm = pad32(c.w_rnn), pad32(c.m_rnn)
        self.host = None            # {checkpoint name: float32 array} of the loaded weights
        self._layout, n = {}, 0
        for name, shape in self._device_shapes().items():
            self._layout[name] = (n, shape)
            n += -(-int(np.prod(shape)) // 64) * 64         # every tensor starts on a 256-byte boundary
        self.flat = torch.zeros(n, dtype=torch.float32, device=self.device)
        self._range = hip.register_param_buffer(self.flat)
        self.d = {name: self.flat[o:o + int(np.prod(shape))].view(shape) for name, (o, shape) in self._layout.items()}
        self._bufs = {}
        self.one = torch.ones(1, dtype=torch.int32, device=self.device)
        self.loaded = False

    def close(self):
        from . import hip
        if self._range is not None:
            hip.release_param_buffer(self._range)
            self._range = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _device_shapes(self):
        """What the kernels read: the backbone's tensors (Backbone.device_tensors), the LSTM kernels cut by input rows and padded
        by gate blocks, the spatial table."""
        c, s = self.cfg, self.cfg.net.device_tensors()
        cw, cm = self.cw, self.cm
        s['vproj/w'], s['vproj/b'] = (1, 1, c.feat_channels, c.v_emb), (c.v_emb,)
        s['embedding'] = (c.vocab_size, c.w_emb)
        s['w/Kx'], s['w/Kh'], s['w/b'] = (c.w_emb, 4 * cw), (cw, 4 * cw), (4 * cw,)
        s['m/Kv'], s['m/Kw'], s['m/Kl'], s['m/Ks'] = (c.v_emb, 4 * cm), (c.w_emb, 4 * cm), (cw, 4 * cm), (8, 4 * cm)
        s['m/Kh'], s['m/b'] = (cm, 4 * cm), (4 * cm,)
        s['proj/w'], s['proj/b'] = (cm,), (1,)
        if c.use_attn:
            s['attn/w'], s['attn/b'] = (cw,), (1,)
        s['spatial'] = (c.feat * c.feat, 8)
        return s

    # ------------------------------------------------------------------ weights
    def load_dict(self, variables):
        """Take {checkpoint name: array}: every variable of MatchConfig.variable_shapes (the LSTM cells also under their older
        names weights / biases); anything else -- optimizer slots, global_step -- is ignored.  ValueError names a variable that
        is missing or has another shape.  The attention's two variables must be there with use_attn and must not without it:
        a head trained to be read through its attention gives nothing meaningful through its last state."""
        import torch
        c, host = self.cfg, {}
        check_attention_variables(variables, c.use_attn)
        c.net.check_variables(variables)
        for name, shape in c.variable_shapes().items():
            src = name
            if src not in variables:
                for new, old in OLD_CELL_NAMES.items():
                    if name.endswith(new) and name[:-len(new)] + old in variables:
                        src = name[:-len(new)] + old
            if src not in variables:        # only a backbone may say that a checkpoint need not hold one of its variables
                host[name] = None if name.startswith(HEAD) else c.net.missing_variable(name, shape)
                if host[name] is None:
                    raise ValueError('the checkpoint has no variable %s' % name)
                continue
            v = np.asarray(variables[src])
            if tuple(v.shape) != tuple(shape):
                raise ValueError('variable %s is %s, the model needs %s' % (src, tuple(v.shape), tuple(shape)))
            host[name] = np.ascontiguousarray(v, dtype=np.float32)
        dev = c.net.device_tensors(host)
        dev.update(pack_head(c, host))
        dev['spatial'] = spatial_features(c.feat, c.feat).reshape(-1, 8)
        assert set(dev) == set(self.d), set(dev) ^ set(self.d)
        for name, v in dev.items():
            self.d[name].copy_(torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).view(self.d[name].shape))
        self.host, self.loaded = host, True

    def init_random(self, seed=0):
        self.load_dict(random_variables(self.cfg, seed))

    def load_tf_checkpoint(self, prefix):
        from . import tf_checkpoint
        if not tf_checkpoint.is_tf_checkpoint(prefix):
            raise ValueError('%s.index: no such TensorFlow checkpoint' % prefix)
        self.load_dict(tf_checkpoint.read_checkpoint(prefix))

    # ------------------------------------------------------------------ buffers
    def _buf(self, tag, shape, dtype=None, zero=False):
        import torch
        key = (tag,) + tuple(shape)
        b = self._bufs.get(key)
        if b is None:
            make = torch.zeros if zero else torch.empty
            b = self._bufs[key] = make(tuple(shape), dtype=dtype or torch.float32, device=self.device)
        return b

    # ------------------------------------------------------------------ backbone
    def backbone(self, x4, keep=None):
        """x4 float [1,S,S,4] (ssc_match_preprocess_u8) -> the visual feature [1,S/8,S/8,feat_channels]: the pass of the
        configuration's backbone (match_backbones.py) on this model's buffers and weights.  keep None: inference, nothing beyond
        the result outlives the pass.  A dict: training -- every output the backward reads goes to a buffer of its own and the dict
        is filled with the record the backward reads (match_backbone_train.py); ValueError from a backbone whose pass cannot be
        kept.  The launches and their operands' values are the same either way."""
        return self.cfg.net.forward(self, x4, keep)

    # ------------------------------------------------------------------ head
    def _lstm_planes(self, tag, rows, C):
        import torch
        from . import hip
        if not hip.lstm_bf(C, 4 * C):
            return None
        return self._buf(tag, (2, hip.lstm_hplanes_floats(rows, C)), zero=True)

    def _cell(self, keep, name, Kh, C, rows, gates_in, c_st, h_st, L, each=None):
        """L steps of an LSTM cell on ``rows`` rows: state t is plane t % P of c_st / h_st [P, rows, C] (state 0 filled by the
        caller), gates_in(t) -> (g1, g2) are the step's two shares of the gates from outside, each(t, h) runs behind step t.
        -> the activated gates [planes, rows, 4C], step t in plane t % planes.  Inference reads no step's gates again: one
        plane, and None where the bf16 step form leaves the store out.  keep: a plane per step, on the bf16 step form too."""
        from . import hip
        if keep is not None:
            acts = self._buf('t_acts_' + name, (self.cfg.max_len, rows, 4 * C))
        else:
            acts = None if hip.lstm_bf(C, 4 * C) else self._buf('acts_' + name, (1, rows, 4 * C))
        hp, P = self._lstm_planes('hp' + name, rows, C), len(c_st)
        for t in range(L):
            a, b = t % P, (t + 1) % P
            g1, g2 = gates_in(t)
            # the step mask ``one``: every row is live (t < seq_len is decided here, on the host)
            hip.lstm_step_fwd(h_st[a], Kh, 4 * C, g1, g2, rows, self.one, rows, c_st[a], rows, C, t > 0, c_st[b], h_st[b],
                              None if acts is None else acts[t % len(acts)],
                              hp_in=None if hp is None or t == 0 else hp[(t - 1) & 1], hp_out=None if hp is None else hp[t & 1])
            if each is not None:
                each(t, h_st[b])
        return acts

    def head(self, feat, tok, seq_len, keep=None):
        """feat float [1,h,w,feat_channels], tok int32 [T] on the device, seq_len on the host -> pred float [h,w].  keep: the cell
        state, the output and the activated gates of every step of both cells stay (MatchTrainer.backward reads them from it)."""
        from . import hip
        from .hip import View
        c, d = self.cfg, self.d
        _, fh, fw, _ = feat.shape
        R, L, cw, cm = fh * fw, int(seq_len), self.cw, self.cm
        assert 1 <= L <= c.max_len and (fh, fw) == (c.feat, c.feat)
        # visual: projection, l2 norm, and its share (with the spatial table's) of the multimodal gates
        vp = self._buf('vproj', (1, fh, fw, c.v_emb))
        hip.conv_forward(View(feat), d['vproj/w'], 1, 0, vp, bias=d['vproj/b'], same=True)
        vis, vis_ss = self._buf('vis', (R, c.v_emb)), self._buf('vis_ss', (R,))
        hip.call('ssc_row_l2norm_fwd', vp, c.v_emb, None, R, c.v_emb, vis, vis_ss)
        gs = self._buf('g_static', (R, 4 * cm))
        hip.matmul(vis, d['m/Kv'], gs)
        hip.matmul(d['spatial'], d['m/Ks'], gs, accumulate=True)
        # words: embedding, the word LSTM over the seq_len real words
        emb = self._buf('emb', (c.max_len, c.w_emb))
        hip.call('ssc_embedding_gather', d['embedding'], tok, L, c.w_emb, emb)
        ew = self._buf('ew', (c.max_len, 4 * cw))
        hip.matmul(emb[:L], d['w/Kx'], ew[:L], bias=d['w/b'])
        cs, hs = self._buf('cw', (c.max_len + 1, cw), zero=True), self._buf('hw', (c.max_len + 1, cw), zero=True)
        own = '' if keep is None else 't_'
        acts_w = self._cell(keep, 'w', d['w/Kh'], cw, 1, lambda t: (ew[t:t + 1], None), cs, hs, L)
        attn = acc = None
        if c.use_attn:      # the weights of the T positions: rows L .. of hs hold an earlier, longer sentence and are not read
            attn = hip.attn_scores_fwd(hs[1:], d['attn/w'], d['attn/b'], c.w_rnn, L, out=self._buf(own + 'attn', (c.max_len,)))
            acc = self._buf(own + 'attn_acc', (R, cm))
        lang, lang_ss = self._buf('lang', (c.max_len, cw)), self._buf('lang_ss', (c.max_len,))
        hip.call('ssc_row_l2norm_fwd', hs[1:], cw, None, L, cw, lang, lang_ss)
        gt = self._buf('g_t', (c.max_len, 4 * cm))
        hip.matmul(emb[:L], d['m/Kw'], gt[:L], bias=d['m/b'])
        hip.matmul(lang[:L], d['m/Kl'], gt[:L], accumulate=True)
        # multimodal LSTM: every location a row, the word's share of the gates the same for all of them.  Inference alternates its
        # states between two planes: step 2 overwrites plane 0, so every pass zeroes it.  keep: a plane per state; state 0 is a
        # zero nobody writes (the steps store 1 .. L)
        P = 2 if keep is None else c.max_len + 1
        ca, ha = (self._buf(own + tag, (P, R, cm), zero=keep is not None) for tag in ('ca', 'ha'))
        if keep is None:
            hip.fill(ca[0], 0.0)
            hip.fill(ha[0], 0.0)
        # acc (+)= attn[t] * m_out[t]; the outputs past L are zero and add nothing
        weigh = None if acc is None else lambda t, h: hip.dev_scaled_add(acc, h, attn, t, overwrite=t == 0)
        acts_m = self._cell(keep, 'm', d['m/Kh'], cm, R, lambda t: (gs, gt[t:t + 1]), ca, ha, L, each=weigh)
        pred = hip.squash_project(ha[L % P] if acc is None else acc, d['proj/w'], d['proj/b'], C=c.m_rnn, out=self._buf(own + 'pred', (R,)))
        if keep is not None:
            keep.update(feat=feat, tok=tok, L=L, R=R, fh=fh, fw=fw, vis=vis, vis_ss=vis_ss, emb=emb, cs=cs, hs=hs, acts_w=acts_w,
                        lang=lang, lang_ss=lang_ss, ca=ca, ha=ha, acts_m=acts_m, attn=attn, acc=acc)
        return pred.view(fh, fw)

    # ------------------------------------------------------------------ the whole pass
    def check_sentence(self, indices, seq_len):
        """The sentence's T indices and its real length -> (int32 [T] on the host, seq_len).  ValueError for another count of
        indices, a length outside 1 .. T or an index outside the vocabulary (ssc_embedding_gather does not clamp)."""
        c = self.cfg
        idx = np.asarray(indices, dtype=np.int64).reshape(-1)
        seq_len = int(seq_len)
        if idx.shape[0] != c.max_len or not 1 <= seq_len <= c.max_len:
            raise ValueError('%d indices with %d real ones: the matcher reads %d, at least one real' % (idx.shape[0], seq_len, c.max_len))
        if idx.min() < 0 or idx.max() >= c.vocab_size:
            raise ValueError('word index %d outside the vocabulary of %d' % (int(idx.max() if idx.max() >= c.vocab_size else idx.min()),
                                                                             c.vocab_size))
        return idx.astype(np.int32), seq_len

    def put_sentence(self, tok):
        """``check_sentence``'s indices into the ``tok`` buffer."""
        import torch
        tok_d = self._buf('tok', (self.cfg.max_len,), torch.int32)
        tok_d.copy_(torch.from_numpy(tok))
        return tok_d

    def put_sketch(self, sketch_u8, check_only=False):
        """sketch uint8 [S,S,3], host or device, into the ``sketch`` buffer (a sketch that already is that buffer stays where it
        is).  RuntimeError without weights, ValueError for another type or shape; check_only: nothing is copied."""
        import torch
        c = self.cfg
        if not self.loaded:
            raise RuntimeError('the matcher has no weights: load_tf_checkpoint or init_random first')
        sk = sketch_u8 if isinstance(sketch_u8, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(sketch_u8))
        if sk.dtype != torch.uint8 or tuple(sk.shape) != (c.size, c.size, 3):
            raise ValueError('the sketch is %s %s, the matcher reads uint8 [%d, %d, 3]' % (sk.dtype, tuple(sk.shape), c.size, c.size))
        skd = self._buf('sketch', (c.size, c.size, 3), torch.uint8)
        if not check_only and skd.data_ptr() != sk.data_ptr():
            skd.copy_(sk)
        return skd

    def upload(self, sketch_u8, indices, seq_len):
        """The inputs into their device buffers; -> (sketch uint8 [S,S,3], tok int32 [T], seq_len).  Both are checked before
        either is copied."""
        self.put_sketch(sketch_u8, check_only=True)
        tok, seq_len = self.check_sentence(indices, seq_len)
        return self.put_sketch(sketch_u8), self.put_sentence(tok), seq_len

    def forward(self, sketch_u8, indices, seq_len):
        """sketch uint8 [S,S,3] (host or device), the sentence's T indices and its real length ->
        (up float [S,S], predicts uint8 [S,S]) on the device, in buffers the next call overwrites."""
        import torch
        from . import hip
        c = self.cfg
        skd, tok, seq_len = self.upload(sketch_u8, indices, seq_len)
        x4, stroke = hip.match_preprocess_u8(skd, out=self._buf('x4', (1, c.size, c.size, 4)),
                                             stroke=self._buf('stroke', (c.size, c.size), torch.uint8))
        pred = self.head(self.backbone(x4), tok, seq_len)
        return hip.match_finish(pred, stroke, up=self._buf('up', (c.size, c.size)),
                                predicts=self._buf('predicts', (c.size, c.size), torch.uint8))

    # ------------------------------------------------------------------ the pass in two halves (match_eval.py)
    def features(self, sketch_u8, keep=None):
        """The half of ``forward`` that does not read the sentence: sketch uint8 [S,S,3] (host or device) -> (feat float
        [1,S/8,S/8,feat_channels], stroke uint8 [S,S]), both in buffers of their own that only the next ``features`` overwrites --
        no ``head``, ``predict`` or ``forward`` call touches them.  keep: ``backbone``'s."""
        import torch
        from . import hip
        c = self.cfg
        skd = self.put_sketch(sketch_u8)
        x4, stroke = hip.match_preprocess_u8(skd, out=self._buf('x4', (1, c.size, c.size, 4)),
                                             stroke=self._buf('stroke_kept', (c.size, c.size), torch.uint8))
        feat = self.backbone(x4, keep)
        if keep is None:    # the map lies in a buffer the next backbone pass reuses (b2s); a kept pass gave it one of its own
            kept = self._buf('feat_kept', tuple(feat.shape))
            kept.copy_(feat)
            feat = kept
        return feat, stroke

    def predict(self, feat, stroke, indices, seq_len):
        """The other half: what ``features`` returned, the sentence's T indices and its real length -> (up float [S,S],
        predicts uint8 [S,S]) in the buffers ``forward`` fills, with the bits ``forward`` gives for that sketch and sentence."""
        import torch
        from . import hip
        c = self.cfg
        tok, seq_len = self.check_sentence(indices, seq_len)
        pred = self.head(feat, self.put_sentence(tok), seq_len)
        return hip.match_finish(pred, stroke, up=self._buf('up', (c.size, c.size)),
                                predicts=self._buf('predicts', (c.size, c.size), torch.uint8))


# ---------------------------------------------------------------------------------------------------------------------------
# the choice of the instances
# ---------------------------------------------------------------------------------------------------------------------------
def pack_masks(boxes, masks, size):
    """-> (uint8 buffer of the small masks one after the other, int64 offsets).  ValueError for a box that is empty or leaves
    the size x size image and for a mask of another shape than its box (both ends of a box belong to it)."""
    boxes = np.asarray(boxes, dtype=np.int32).reshape(-1, 4)
    if len(boxes) != len(masks) or len(boxes) == 0:
        raise ValueError('%d boxes and %d masks' % (len(boxes), len(masks)))
    offsets, parts, n = [], [], 0
    for k, ((y1, x1, y2, x2), m) in enumerate(zip(boxes.tolist(), masks)):
        m = np.ascontiguousarray(m, dtype=np.uint8)
        if y1 < 0 or x1 < 0 or y2 < y1 or x2 < x1 or y2 >= size or x2 >= size:
            raise ValueError('the box (%d, %d, %d, %d) of instance %d is empty or leaves the %d x %d image' % (y1, x1, y2, x2, k, size, size))
        if m.shape != (y2 - y1 + 1, x2 - x1 + 1):
            raise ValueError('the mask of instance %d is %s, its box needs %s' % (k, m.shape, (y2 - y1 + 1, x2 - x1 + 1)))
        offsets.append(n)
        parts.append(m.reshape(-1))
        n += m.size
    return np.concatenate(parts), np.asarray(offsets, dtype=np.int64)


def select_instances(counts):
    """int64 [N,2] = (intersection, sum of the mask's bytes) -> (matched indices in instance order, float64 scores): the
    quotient in float64, matched where it is above 0.5; an empty mask (0 / 0, nan) is not matched."""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1, 2)
    with np.errstate(divide='ignore', invalid='ignore'):
        scores = counts[:, 0].astype(np.float64) / counts[:, 1].astype(np.float64)
    return [int(k) for k in np.nonzero(scores > OCCUPIED_THRESH)[0]], scores


def _counts(predicts_d, buf, boxes, offsets):
    import torch
    from . import hip
    dev = predicts_d.device
    counts = hip.instance_occupancy(predicts_d, torch.from_numpy(buf).to(dev),
                                    torch.from_numpy(np.ascontiguousarray(boxes, dtype=np.int32).reshape(-1, 4)).to(dev),
                                    torch.from_numpy(offsets).to(dev)).cpu().numpy()
    if (counts < 0).any():
        raise RuntimeError('ssc_instance_occupancy refused instance %d' % int(np.nonzero(counts[:, 0] < 0)[0][0]))
    return counts


def instance_counts(predicts_d, boxes, masks):
    """predicts uint8 [S,S] on the device -> int64 [N,2] on the host (ssc_instance_occupancy)."""
    buf, offsets = pack_masks(boxes, masks, int(predicts_d.shape[0]))
    return _counts(predicts_d, buf, boxes, offsets)


def match_instances(model, scene, text, vocab):
    """scene: what fg_scene.load_instances returns (sketch, boxes, masks, class_ids) at the model's size ->
    (matched instance indices, float64 occupancy of every instance, info: tokens, indices, seq_len, counts, up, predicts).
    A bad sentence or a bad box is refused before any launch."""
    T = model.cfg.max_len
    indices, seq_len = preprocess_sentence(text, vocab, T)
    buf, offsets = pack_masks(scene['boxes'], scene['masks'], model.cfg.size)
    up, predicts = model.forward(scene['sketch'], indices, seq_len)
    counts = _counts(predicts, buf, scene['boxes'], offsets)
    matched, scores = select_instances(counts)
    info = {'tokens': sentence_tokens(text)[:T], 'indices': list(indices), 'seq_len': seq_len, 'counts': counts,
            'up': up.cpu().numpy(), 'predicts': predicts.cpu().numpy()}
    if model.cfg.use_attn:      # the T weights of the pass, the padded positions' included: they sum to 1
        info['attention'] = model._buf('attn', (T,)).cpu().numpy()
    return matched, scores, info


def resolve_snapshot(path):
    """A checkpoint prefix, or a directory with TensorFlow's ``checkpoint`` file -> the prefix.  ValueError when neither."""
    if os.path.exists(path + '.index'):
        return path
    idx = os.path.join(path, 'checkpoint')
    if os.path.isdir(path) and os.path.exists(idx):
        with open(idx) as f:
            line = f.readline()
        if '"' in line:
            prefix = os.path.join(path, os.path.basename(line.split('"')[1]))
            if os.path.exists(prefix + '.index'):
                return prefix
    raise ValueError('--snapshot %r: neither a checkpoint prefix (<prefix>.index) nor a directory whose checkpoint file names one' % path)
