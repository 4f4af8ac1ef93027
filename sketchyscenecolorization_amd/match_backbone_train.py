"""Training the matcher's backbone beside its fusion head (match_main.py --train_backbone 1; RMI_model.py::train_op with
train_fusion_var_only=False, RMI_model.py:320-330): every filter of the DeepLab-ResNet (DeepLabBackbone.trained_variable_names:
ResNet/*/DW) learns, through norms that stay as they were loaded -- beta, gamma, factor, mean and variance are trainable=False and
bn=False reads the stored moments (deeplab_model.py:176-231).  DESIGN.md section 8.10.

    forward   backbone_train: MatchModel.backbone with keep (DeepLabBackbone.forward; the feature map has inference's bits): every
              unit's raw conv outputs r1, r2, r3, sc and its merged output in buffers of their own
    backward  MatchTrainer.backward with dfeat = dvp . DW^T -> ssc_space_to_batch(2) per doubling of the rate (the backward of
              the final ungroup) -> per unit, last to first: ssc_unit_merge_bwd (the closing relu, both branches), conv_wgrad /
              conv_dgrad through block_3, block_2, block_1 with ssc_frozen_act_bwd between them (the consumer-side views are the
              filter gradients' x), the shortcut's gradient added by the last conv_dgrad (identity) or by a second one (projection);
              the two stride-2 1x1 convs of group_3_0: the stride-1 gradient on the low lattice, then ssc_zero_stuff2;
              ssc_batch_to_space(2) where the forward regrouped -> ssc_max_pool3s2_bwd -> conv_wgrad of the 7x7 stride-2 filter
    update    ssc_l2_reg and ssc_adam_tf (the head's step size, scale 1: no backbone variable is a 'biases') on every DW span of
              MatchModel.flat; the [a | b] norm tables between the spans are not touched; hip.refresh_splits

Not here: batch-statistics norms (bn=True), training the norm parameters, a captured step, cached features (they are those of the
initial backbone)."""
import numpy as np

from . import match_train, matching
from .match_train import MatchTrainer


def backbone_variable_names(config):
    """The trained backbone variables under their checkpoint names, in variable_shapes' order: the backbone object's (for the
    DeepLab-ResNet its filters; ValueError from a backbone without a backward)."""
    return config.net.trained_variable_names()


def trained_variable_names(config, train_backbone):
    """What an iteration updates: the head, and with ``train_backbone`` the backbone's filters in front of it."""
    return (backbone_variable_names(config) if train_backbone else []) + match_train.head_variable_names(config)


def unit_geometry(config):
    """[(scope, cin, cout, stride, space_to_batch(2) moves in front of the unit, shape of its input, shape of its output)] as
    ``backbone_train`` runs the units: groups 4 and 5 in the space-to-batch layout."""
    n, h, cur, out = 1, config.size // 4, 1, []
    for scope, cin, cout, stride, rate in config.net.unit_list():
        moves = 0
        while cur < rate:
            n, h, cur, moves = n * 4, h // 2, cur * 2, moves + 1
        oh = -(-h // stride)
        out.append((scope, cin, cout, stride, moves, (n, h, h, cin), (n, oh, oh, cout)))
        h = oh
    return out


def _gkey(tag, shape):
    shape = tuple(int(v) for v in shape)
    return 'bb/%s%r' % (tag, shape), shape


def forward_buffer_shapes(config):
    """{tag: shape} of every float32 buffer ``backbone_train`` keeps for the backward, by shapes alone."""
    c, s = config, {}
    s['bt/conv1'] = (1, c.size // 2, c.size // 2, c.filters[0])
    s['bt/pool'] = (1, c.size // 4, c.size // 4, c.filters[0])
    cur = 1
    for scope, cin, cout, _stride, moves, xs, (n, oh, ow, _c) in unit_geometry(c):
        for m in range(moves):
            cur *= 2
            s['bt/s2b%d' % cur] = (xs[0] >> (2 * (moves - 1 - m)), xs[1] << (moves - 1 - m), xs[2] << (moves - 1 - m), cin)
        for tag, ch in (('r1', cout // 4), ('r2', cout // 4), ('r3', cout), ('out', cout)) + ((('sc', cout),) if cin != cout else ()):
            s['bt/%s/%s' % (scope, tag)] = (n, oh, ow, ch)
    while cur > 1:
        n, oh, ow, cur = n // 4, oh * 2, ow * 2, cur // 2
        s['bt/b2s%d' % cur] = (n, oh, ow, c.feat_channels)
    return s


def backward_buffer_shapes(config):
    """{tag: shape} of the scratch of ``backbone_backward``: a buffer is shared by every unit that asks for its tag and shape."""
    c, s = config, {}
    geo = unit_geometry(c)

    def add(tag, shape):
        key, shape = _gkey(tag, shape)
        s[key] = shape
    s['bb/dfeat'] = (1, c.feat, c.feat, c.feat_channels)
    n, h, w, ch = s['bb/dfeat']
    while n < geo[-1][6][0]:
        n, h, w = n * 4, h // 2, w // 2
        add('move', (n, h, w, ch))
    for k, (_scope, cin, cout, stride, moves, xs, os_) in enumerate(geo):
        add('g%d' % (k & 1), xs)
        add('dr3', os_)
        if cin != cout:
            add('dsc', os_)
        add('g12', os_[:3] + (cout // 4,))
        add('g12b', os_[:3] + (cout // 4,))
        if stride != 1:
            add('low', os_[:3] + (cin,))
        n, h, w, ch = xs
        for _ in range(moves):
            n, h, w = n // 4, h * 2, w * 2
            add('move', (n, h, w, ch))
    s['bb/dr0'] = (1, c.size // 2, c.size // 2, c.filters[0])
    return s


def training_bytes(config):
    """-> (bytes of the kept activations, bytes of the backward's scratch, bytes of the gradient and the two Adam slot buffers)."""
    n = lambda shapes: 4 * sum(int(np.prod(v)) for v in shapes.values())
    span = sum(-(-int(np.prod(shape)) // 64) * 64 for shape in config.net.device_tensors().values())      # as MatchModel lays them out
    return n(forward_buffer_shapes(config)), n(backward_buffer_shapes(config)), 3 * 4 * span


def check_budget(config, free_bytes, beside=0):
    """ValueError with the bytes when what --train_backbone 1 adds (beside ``beside`` bytes of caches) is more than half of the free
    device memory.  -> the three figures of ``training_bytes``."""
    act, scratch, slots = training_bytes(config)
    need = act + scratch + slots + int(beside)
    if need > free_bytes // 2:
        raise ValueError('--train_backbone 1 keeps %d bytes of activations, %d of gradient scratch and %d of gradient and Adam slots '
                         '(%d with the caches): more than half of the %d bytes free on the device; train at a smaller --scene_size '
                         'or with --train_backbone 0' % (act, scratch, slots, need, free_bytes))
    return act, scratch, slots


class BackboneMatchTrainer(MatchTrainer):
    """MatchTrainer whose iteration also differentiates the backbone and updates its filters.  ``bg``, ``bm`` and ``bv`` are
    views into the backbone's gradient buffer and Adam slot buffers by checkpoint name."""

    def __init__(self, model, weight_decay=5e-4):
        MatchTrainer.__init__(self, model, weight_decay)
        lay = model._layout
        self.b_names = backbone_variable_names(self.cfg)
        self.b_hi = self.lo             # the backbone is the stretch of the flat buffer in front of the head
        inside = [n for n, (o, _s) in lay.items() if o < self.b_hi]
        assert inside == list(self.cfg.net.device_tensors()) and [n for n in inside if n in self.b_names] == self.b_names, inside
        self.b_params, (self.b_grad, self.b_adam_m, self.b_adam_v), self.b_spans, (self.bg, self.bm, self.bv) = \
            match_train.trained_stretch(model, self.b_names, 0, self.b_hi)
        self._kept = None           # what MatchModel.backbone kept of the latest pass: units, x4, r0
        self.on_part = None         # a callable(name), called behind each part of backbone_backward (scripts/match_backbone_train_rate.py)

    # ------------------------------------------------------------------ forward
    def _bbuf(self, tag, shape):
        return self.model._buf(tag, shape)

    def reserve(self):
        """Allocate now every buffer the forward keeps and the backward uses (they are allocated at first use otherwise)."""
        for shapes in (forward_buffer_shapes(self.cfg), backward_buffer_shapes(self.cfg)):
            for tag, shape in shapes.items():
                self._bbuf(tag, shape)

    def backbone_train(self, x4):
        """MatchModel.backbone on x4 float [1,S,S,4] with every output kept for ``backbone_backward`` (the buffers of
        ``forward_buffer_shapes``): the same pass, so the feature map has its bits."""
        kept = {}
        feat = self.model.backbone(x4, keep=kept)
        self._kept = kept
        return feat

    def _features(self, sketch):
        """MatchModel.features with the backbone's outputs kept; the feature map stays where the pass left it."""
        kept = {}
        feat = self.model.features(sketch, keep=kept)[0]
        self._kept = kept
        return feat

    def step(self, scene, lut, tok, seq_len, lr):
        if 'feat_d' in scene:
            raise ValueError('a cached feature is that of the initial backbone: the step that trains the backbone takes the sketch')
        return MatchTrainer.step(self, scene, lut, tok, seq_len, lr)

    # ------------------------------------------------------------------ backward
    def backward(self, dpred, dfeat=None):
        """The head's backward, then the backbone's from the gradient on the feature map: fills the gradient of every trained
        tensor of both."""
        c = self.cfg
        if self._kept is None:
            raise RuntimeError('backward without a backbone_train before it')
        if dfeat is None:
            dfeat = self._bbuf('bb/dfeat', (1, c.feat, c.feat, c.feat_channels))
        MatchTrainer.backward(self, dpred, dfeat)
        self.backbone_backward(dfeat)

    def _gbuf(self, tag, shape):
        return self._bbuf(*_gkey(tag, shape))

    def backbone_backward(self, dfeat):
        """dfeat float [1,S/8,S/8,feat_channels]: the gradient on ``backbone_train``'s feature map.  Fills ``bg``."""
        from . import hip
        from .hip import ACT_RELU, View
        c, d, bg, net = self.cfg, self.model.d, self.bg, self.cfg.net
        units = self._kept['units']
        # the scratch buffers are reused from unit to unit: every launch, the filter gradients included, is on this one stream
        assert hip.WGRAD_STREAM is None
        # the final ungroup backwards: into the layout of the last unit
        g = dfeat
        nb = units[-1]['out'].shape[0]
        while g.shape[0] < nb:
            n, h, w, ch = g.shape
            g = hip.space_to_batch(g, 2, out=self._gbuf('move', (n * 4, h // 2, w // 2, ch)))
        for k in range(len(units) - 1, -1, -1):
            u = units[k]
            scope, stride, x, out = u['scope'], u['stride'], u['x'], u['out']
            n, oh, ow, cout = out.shape
            cin = x.shape[3]
            ab1, ab2, ab3 = (d['%s/block_%d/bn' % (scope, j)] for j in (1, 2, 3))
            w1, w2, w3 = (d['%s/block_%d/conv/DW' % (scope, j)] for j in (1, 2, 3))
            proj = u['sc'] is not None
            dx = self._gbuf('g%d' % (k & 1), x.shape)
            assert dx.data_ptr() != g.data_ptr()
            dr3 = self._gbuf('dr3', out.shape)
            # the closing relu: dr3, and the shortcut's share (d sc, or dx itself for the identity)
            dsc = self._gbuf('dsc', out.shape) if proj else dx
            hip.unit_merge_bwd(g, out, ab3, d[scope + '/block_add/bn'] if proj else None, dr3=dr3, d2=dsc)
            # block_3 (1x1), block_2 (3x3 SAME), block_1 (1x1, the unit's stride)
            hip.conv_wgrad(View(u['r2'], None, ab2, ACT_RELU), View(dr3), bg[scope + '/block_3/conv/DW'], 1, 0)
            g2 = self._gbuf('g12', u['r2'].shape)
            hip.conv_dgrad(View(dr3), w3, 1, 0, g2)
            hip.frozen_act_bwd(g2, u['r2'], ab2, out=g2)
            hip.conv_wgrad(View(u['r1'], None, ab1, ACT_RELU), View(g2), bg[scope + '/block_2/conv/DW'], 1, 1)
            g1 = self._gbuf('g12b', u['r1'].shape)
            hip.conv_dgrad(View(g2), w2, 1, 1, g1)
            hip.frozen_act_bwd(g1, u['r1'], ab1, out=g1)
            hip.conv_wgrad(View(x), View(g1), bg[scope + '/block_1/conv/DW'], stride, 0)
            if proj:
                hip.conv_wgrad(View(x), View(dsc), bg[scope + '/block_add/conv/DW'], stride, 0)
                # a 1x1 conv of stride 2 reads the even pixels: the stride-1 gradient on that lattice, zero elsewhere
                low = dx if stride == 1 else self._gbuf('low', (n, oh, ow, cin))
                hip.conv_dgrad(View(g1), w1, 1, 0, low)
                hip.conv_dgrad(View(dsc), d[scope + '/block_add/conv/DW'], 1, 0, low, accumulate=True)
                if stride != 1:
                    assert stride == 2
                    hip.zero_stuff2(low, dx)
            else:
                hip.conv_dgrad(View(g1), w1, 1, 0, dx, accumulate=True)     # onto the identity's share
            g = dx
            for _ in range(u['regroups']):      # the backward of a regroup in front of this unit
                nbb, h, w, ch = g.shape
                g = hip.batch_to_space(g, 2, out=self._gbuf('move', (nbb // 4, h * 2, w * 2, ch)))
            if self.on_part is not None and scope.endswith('_0'):
                self.on_part(scope.rsplit('/', 1)[1][:-2])         # 'group_5' .. 'group_2': the group's units are behind us
        # the pool with conv1's relu, then conv1's filter: 3 real channels of the 4-channel input, SAME pad (2, 3)
        r0 = self._kept['r0']
        dr0 = hip.max_pool3s2_bwd(g, r0, d[net.CONV1_NORM], out=self._bbuf('bb/dr0', r0.shape))
        hip.conv_wgrad(View(self._kept['x4']), View(dr0), bg[net.CONV1], 2, hip.same_pad_before(c.size, 7, 2))
        hip.join_wgrad()
        if self.on_part is not None:
            self.on_part('pool and conv1')

    # ------------------------------------------------------------------ optimiser
    def apply(self, lr):
        """MatchTrainer.apply on the head, then the same on the backbone's filters with the head's step size: every DW is
        regularised and none is a 'biases'."""
        MatchTrainer.apply(self, lr)
        match_train.apply_adam(self.b_params, self.b_grad, self.b_adam_m, self.b_adam_v, self.b_spans, {n: n for n in self.b_names},
                               match_train.adam_step_size(lr, self.step_count), self.weight_decay)

    # ------------------------------------------------------------------ weights in and out
    def export_variables(self):
        """{checkpoint name: array}: the head and the backbone's filters from the device, the norms as they were loaded."""
        out = MatchTrainer.export_variables(self)
        out.update(self._export_backbone(self.model.d))
        return out

    def _export_backbone(self, views):
        return {n: views[n].detach().cpu().numpy().copy() for n in self.b_names}

    def export_backbone_gradients(self):
        return self._export_backbone(self.bg)

    def snapshot_tensors(self):
        out = MatchTrainer.snapshot_tensors(self)
        match_train.slots_to_snapshot(out, self.bm, self.bv, self._export_backbone)
        return out

    def load_slots(self, tensors, step):
        match_train.slots_from_snapshot(tensors, self.bm, self.bv, self.b_names, dict,
                                        'it was written by a run with --train_backbone 0 (or not by training); resume it with '
                                        '--train_backbone 0')
        MatchTrainer.load_slots(self, tensors, step)
