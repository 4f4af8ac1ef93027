"""Training the matcher's backbone beside its fusion head (match_main.py --train_backbone 1; RMI_model.py::train_op with
train_fusion_var_only=False, RMI_model.py:320-330): every ResNet/*/DW filter of the DeepLab-ResNet learns, through norms that stay
as they were loaded -- beta, gamma, factor, mean and variance are trainable=False and bn=False reads the stored moments
(deeplab_model.py:176-231).  DESIGN.md section 8.10.

    forward   backbone_train: the launches of MatchModel.backbone on the same operands (the feature map has its bits), every
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
from .match_train import BETA1, BETA2, EPSILON, MatchTrainer


def backbone_variable_names(config):
    """The trained backbone variables under their checkpoint names, in variable_shapes' order: the ResNet/*/DW filters."""
    return [n for n in config.variable_shapes() if n.startswith('ResNet/') and n.endswith('/DW')]


def trained_variable_names(config, train_backbone):
    """What an iteration updates: the head, and with ``train_backbone`` the backbone's filters in front of it."""
    return (backbone_variable_names(config) if train_backbone else []) + match_train.head_variable_names(config)


def unit_geometry(config):
    """[(scope, cin, cout, stride, space_to_batch(2) moves in front of the unit, shape of its input, shape of its output)] as
    ``backbone_train`` runs the units: groups 4 and 5 in the space-to-batch layout."""
    n, h, cur, out = 1, config.size // 4, 1, []
    for scope, cin, cout, stride, rate in config.unit_list():
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
        s['bt/b2s%d' % cur] = (n, oh, ow, c.filters[4])
    return s


def backward_buffer_shapes(config):
    """{tag: shape} of the scratch of ``backbone_backward``: a buffer is shared by every unit that asks for its tag and shape."""
    c, s = config, {}
    geo = unit_geometry(c)

    def add(tag, shape):
        key, shape = _gkey(tag, shape)
        s[key] = shape
    s['bb/dfeat'] = (1, c.feat, c.feat, c.filters[4])
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
    span = 0
    for name, shape in config.variable_shapes().items():
        scope, leaf = name.rsplit('/', 1)
        if name.startswith('ResNet/') and leaf in ('DW', 'gamma'):
            span += -(-(int(np.prod(shape)) * (2 if leaf == 'gamma' else 1)) // 64) * 64
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
        import torch
        MatchTrainer.__init__(self, model, weight_decay)
        lay = model._layout
        self.b_names = backbone_variable_names(self.cfg)
        self.b_hi = self.lo             # the backbone is the stretch of the flat buffer in front of the head
        inside = [n for n, (o, _s) in lay.items() if o < self.b_hi]
        assert all(n.startswith('ResNet/') for n in inside) and [n for n in inside if n.endswith('/DW')] == self.b_names, inside
        self.b_params = model.flat[:self.b_hi]
        self.b_grad, self.b_adam_m, self.b_adam_v = (torch.zeros(self.b_hi, dtype=torch.float32, device=model.device) for _ in range(3))
        order = list(lay)
        self.b_spans = {}
        for name in self.b_names:
            o, shape = lay[name]
            self.b_spans[name] = (o, int(np.prod(shape)), lay[order[order.index(name) + 1]][0] - o, shape)
        self.bg, self.bm, self.bv = ({n: buf[o:o + size].view(shape) for n, (o, size, _p, shape) in self.b_spans.items()}
                                     for buf in (self.b_grad, self.b_adam_m, self.b_adam_v))
        self._units = None
        self.on_part = None         # a callable(name), called behind each part of backbone_backward (scripts/match_backbone_train_rate.py)

    # ------------------------------------------------------------------ forward
    def _bbuf(self, tag, shape):
        return self.model._buf(tag, shape)

    def reserve(self):
        """Allocate now every buffer the forward keeps and the backward uses (they are allocated at first use otherwise)."""
        for shapes in (forward_buffer_shapes(self.cfg), backward_buffer_shapes(self.cfg)):
            for tag, shape in shapes.items():
                self._bbuf(tag, shape)

    def unit_train(self, x, scope, stride):
        """MatchModel.unit with every output in a buffer of the unit's own.  -> the record ``backward`` reads."""
        from . import hip
        from .hip import ACT_RELU, View
        d = self.model.d
        n, h, w, cin = x.shape
        oh, ow = -(-h // stride), -(-w // stride)
        w1, w2, w3 = (d['%s/block_%d/conv/DW' % (scope, k)] for k in (1, 2, 3))
        c4, cout = w1.shape[3], w3.shape[3]
        t = 'bt/%s/' % scope
        r1 = self._bbuf(t + 'r1', (n, oh, ow, c4))
        hip.conv_forward(View(x), w1, stride, 0, r1, same=True)
        r2 = self._bbuf(t + 'r2', (n, oh, ow, c4))
        hip.conv_forward(View(r1, None, d[scope + '/block_1/bn'], ACT_RELU), w2, 1, 0, r2, same=True)
        r3 = self._bbuf(t + 'r3', (n, oh, ow, cout))
        hip.conv_forward(View(r2, None, d[scope + '/block_2/bn'], ACT_RELU), w3, 1, 0, r3, same=True)
        out = self._bbuf(t + 'out', (n, oh, ow, cout))
        wadd = d.get(scope + '/block_add/conv/DW')
        sc = None
        if wadd is not None:
            sc = self._bbuf(t + 'sc', (n, oh, ow, cout))
            hip.conv_forward(View(x), wadd, stride, 0, sc, same=True)
            hip.call('ssc_residual_merge', r3, d[scope + '/block_3/bn'], sc, d[scope + '/block_add/bn'], ACT_RELU, out,
                     n * oh * ow, cout)
        else:
            assert cin == cout and stride == 1, (scope, cin, cout, stride)
            hip.call('ssc_residual_merge', r3, d[scope + '/block_3/bn'], x, None, ACT_RELU, out, n * oh * ow, cout)
        return dict(scope=scope, stride=stride, x=x, r1=r1, r2=r2, r3=r3, sc=sc, out=out, regroups=0)

    def backbone_train(self, x4):
        """x4 float [1,S,S,4] -> the visual feature [1,S/8,S/8,filters[4]], with the bits of MatchModel.backbone."""
        from . import hip
        from .hip import View
        c, d = self.cfg, self.model.d
        s = c.size
        r0 = self._bbuf('bt/conv1', (1, s // 2, s // 2, c.filters[0]))
        hip.conv_forward(View(x4), d['ResNet/group_1/conv1/DW'], 2, 0, r0, same=True)
        x = hip.max_pool3s2(r0, d['ResNet/group_1/bn_conv1'], out=self._bbuf('bt/pool', (1, s // 4, s // 4, c.filters[0])))
        cur, units = 1, []
        for scope, _cin, _cout, stride, rate in c.unit_list():
            regroups = 0
            while cur < rate:
                n, h, w, ch = x.shape
                cur *= 2
                x = hip.space_to_batch(x, 2, out=self._bbuf('bt/s2b%d' % cur, (n * 4, h // 2, w // 2, ch)))
                regroups += 1
            rec = self.unit_train(x, scope, stride)
            rec['regroups'] = regroups          # how many space_to_batch(2) ran in front of this unit
            units.append(rec)
            x = rec['out']
        while cur > 1:
            nb, h, w, ch = x.shape
            cur //= 2
            x = hip.batch_to_space(x, 2, out=self._bbuf('bt/b2s%d' % cur, (nb // 4, h * 2, w * 2, ch)))
        self._units, self._x4, self._r0 = units, x4, r0
        return x

    def _features(self, sketch):
        """MatchModel.features with ``backbone_train`` in the place of ``backbone``."""
        import torch
        from . import hip
        mdl, c = self.model, self.cfg
        sk = sketch if isinstance(sketch, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(sketch))
        if sk.dtype != torch.uint8 or tuple(sk.shape) != (c.size, c.size, 3):
            raise ValueError('the sketch is %s %s, the matcher reads uint8 [%d, %d, 3]' % (sk.dtype, tuple(sk.shape), c.size, c.size))
        skd = mdl._buf('sketch', (c.size, c.size, 3), torch.uint8)
        if skd.data_ptr() != sk.data_ptr():
            skd.copy_(sk)
        x4, _ = hip.match_preprocess_u8(skd, out=mdl._buf('x4', (1, c.size, c.size, 4)),
                                        stroke=mdl._buf('stroke_kept', (c.size, c.size), torch.uint8))
        return self.backbone_train(x4)

    def step(self, scene, lut, tok, seq_len, lr):
        if 'feat_d' in scene:
            raise ValueError('a cached feature is that of the initial backbone: the step that trains the backbone takes the sketch')
        return MatchTrainer.step(self, scene, lut, tok, seq_len, lr)

    # ------------------------------------------------------------------ backward
    def backward(self, dpred, dfeat=None):
        """The head's backward, then the backbone's from the gradient on the feature map: fills the gradient of every trained
        tensor of both."""
        c = self.cfg
        if self._units is None:
            raise RuntimeError('backward without a backbone_train before it')
        if dfeat is None:
            dfeat = self._bbuf('bb/dfeat', (1, c.feat, c.feat, c.filters[4]))
        MatchTrainer.backward(self, dpred, dfeat)
        self.backbone_backward(dfeat)

    def _gbuf(self, tag, shape):
        return self._bbuf(*_gkey(tag, shape))

    def backbone_backward(self, dfeat):
        """dfeat float [1,S/8,S/8,filters[4]]: the gradient on ``backbone_train``'s feature map.  Fills ``bg``."""
        from . import hip
        from .hip import ACT_RELU, View
        c, d, bg = self.cfg, self.model.d, self.bg
        units = self._units
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
        r0 = self._r0
        dr0 = hip.max_pool3s2_bwd(g, r0, d['ResNet/group_1/bn_conv1'], out=self._bbuf('bb/dr0', r0.shape))
        hip.conv_wgrad(View(self._x4), View(dr0), bg['ResNet/group_1/conv1/DW'], 2, hip.same_pad_before(c.size, 7, 2))
        hip.join_wgrad()
        if self.on_part is not None:
            self.on_part('pool and conv1')

    # ------------------------------------------------------------------ optimiser
    def apply(self, lr):
        """MatchTrainer.apply on the head, then the same on the backbone's filters: the regulariser on every DW, TF's Adam with
        the head's step size and scale 1, the bf16 planes of what changed."""
        from . import hip
        MatchTrainer.apply(self, lr)
        lr_t = match_train.adam_step_size(lr, self.step_count)
        if self.weight_decay != 0.0:
            for _name, (o, size, _padded, _shape) in self.b_spans.items():
                hip.call('ssc_l2_reg', self.b_params[o:o + size], size, self.weight_decay, None, self.b_grad[o:o + size])
        for _name, (o, _size, padded, _shape) in self.b_spans.items():
            hip.call('ssc_adam_tf', self.b_params[o:o + padded], self.b_grad[o:o + padded], self.b_adam_m[o:o + padded],
                     self.b_adam_v[o:o + padded], padded, lr_t, None, BETA1, BETA2, EPSILON, 1.0)
        hip.refresh_splits(self.b_params)

    # ------------------------------------------------------------------ weights in and out
    def export_variables(self):
        """{checkpoint name: array}: the head and the backbone's filters from the device, the norms as they were loaded."""
        out = MatchTrainer.export_variables(self)
        for name in self.b_names:
            out[name] = self.model.d[name].detach().cpu().numpy().copy()
        return out

    def export_backbone_gradients(self):
        return {n: self.bg[n].detach().cpu().numpy().copy() for n in self.b_names}

    def snapshot_tensors(self):
        out = MatchTrainer.snapshot_tensors(self)
        for suffix, views in (('/Adam', self.bm), ('/Adam_1', self.bv)):
            for name in self.b_names:
                out[name + suffix] = views[name].detach().cpu().numpy().copy()
        return out

    def load_slots(self, tensors, step):
        import torch
        for suffix, views in (('/Adam', self.bm), ('/Adam_1', self.bv)):
            for name in self.b_names:
                if name + suffix not in tensors:
                    raise ValueError('the snapshot has no %s: it was written by a run with --train_backbone 0 (or not by training); '
                                     'resume it with --train_backbone 0' % (name + suffix))
                a = np.ascontiguousarray(tensors[name + suffix], dtype=np.float32)
                if a.shape != tuple(views[name].shape):
                    raise ValueError('%s is %s, the model needs %s' % (name + suffix, a.shape, tuple(views[name].shape)))
                views[name].copy_(torch.from_numpy(a))
        MatchTrainer.load_slots(self, tensors, step)
