"""The backbones of the instance matcher (matching.py): everything that depends on which network turns the sketch into the visual
feature map lives here, once per backbone -- its checkpoint scope and variables, its released widths, the checks of its sizes, what
of a checkpoint goes to the device and in which form, its forward pass on a MatchModel's buffers and weights, the scratch memory it
reserves, and whether its pass can be kept for a backward.  MatchConfig makes the object from (size, units, filters) on the host
(``MatchConfig.net``); torch and the HIP binding are imported only when a pass is asked for.

    DeepLabBackbone  'deeplab': the DeepLab-ResNet of deeplab_model.py (is_intermediate, frozen norms).  DESIGN.md section 8.6; its
                     kept pass is what match_backbone_train.py differentiates (section 8.10).
    SegNetBackbone   'segnet': segnet_model.py (is_intermediate), the norms of the one image.  DESIGN.md section 8.12.

What a further backbone has to provide: DESIGN.md section 8.13."""
import numpy as np

NORM_EPS = 0.001
NORM_PARTS = ('beta', 'gamma', 'factor', 'mean', 'variance')
# tf.contrib.layers.batch_norm with its defaults (segnet_model.py:133): no gamma; the moving moments exist and are never read
SEGNET_NORM_PARTS = ('beta', 'moving_mean', 'moving_variance')


def fold_norm(beta, gamma, factor, mean, variance):
    """The frozen norm y = (x - mean/factor) * rsqrt(variance/factor + 0.001) * gamma + beta as y = a*x + b: float32 [2C] =
    [a | b], worked out in float64."""
    beta, gamma, mean, variance = (np.asarray(v, np.float64).reshape(-1) for v in (beta, gamma, mean, variance))
    factor = float(np.asarray(factor, np.float64).reshape(-1)[0])
    a = gamma / np.sqrt(variance / factor + NORM_EPS)
    return np.concatenate([a, beta - mean / factor * a]).astype(np.float32)


class Backbone(object):
    """What MatchConfig, MatchModel, the trainers and match_main.py ask of a backbone.  A subclass sets ``name`` (the value of
    --weights), ``title``, ``scope`` (of its variables in a checkpoint), ``released`` (the widths of the released model),
    ``model_name`` (of snapshots and result files), ``size_reason`` and ``trainable``, and writes ``widths``, ``feat_channels``,
    ``variable_shapes``, ``device_tensors`` and ``forward``."""
    trainable = False       # whether ``forward`` can keep its pass for a backward

    def __init__(self, size, units, filters=None):
        if filters is None:
            filters = self.released
        self.size, self.units, self.filters = int(size), tuple(int(u) for u in units), tuple(int(f) for f in filters)
        if self.size < 32 or self.size % 32:
            raise ValueError('size %d: the matcher needs a multiple of 32 (%s)' % (self.size, self.size_reason))
        if len(self.units) != 4 or min(self.units) < 1 or len(self.filters) != 5:
            raise ValueError('units %r / filters %r: four groups of at least one unit, five widths' % (self.units, self.filters))

    def check_widths(self, more=()):
        """ValueError for a channel count of ``widths`` or of ``more`` [(what, count)] that is no multiple of 4."""
        for name, c in self.widths() + list(more):
            if c < 4 or c % 4:
                raise ValueError('%s = %d: every channel count must be a multiple of 4' % (name, c))
        if any(f % 4 for f in self.filters):
            raise ValueError('filters %r: every channel count must be a multiple of 4' % (self.filters,))

    def missing_variable(self, name, shape):
        """The value of a variable that a checkpoint may lack, or None: it must be there."""
        return None

    def check_variables(self, names):
        """names: the variable names of a checkpoint (any container).  ValueError when it holds the variables of another
        backbone: a head trained on one backbone's feature map gives nothing meaningful on another's.  Names the flag and a
        variable."""
        for other in BACKBONES.values():
            if other.name != self.name:
                found = sorted(n for n in names if n.startswith(other.scope))
                if found:
                    raise ValueError("the checkpoint holds %s: it belongs to the %s backbone (--weights %s), not to --weights %s"
                                     % (found[0], other.name, other.name, self.name))

    def scratch_bytes(self):
        """What ``forward`` allocates at its first pass beyond the weights and the buffers it shares; 0: nothing to speak of."""
        return 0

    def check_scratch(self, free):
        """``scratch_bytes`` against ``free``, the bytes free on the device: -> the bytes; ValueError when they are more than half
        of what is free."""
        need = self.scratch_bytes()
        if need > int(free) // 2:
            raise ValueError('the %s backbone needs %d bytes of scratch memory at size %d, more than half of the %d bytes free on '
                             'the device' % (self.title, need, self.size, int(free)))
        return need

    def trained_variable_names(self):
        """The checkpoint names of the variables that training the backbone updates, in variable_shapes' order.  ValueError for a
        backbone whose pass cannot be kept: the one refusal behind ``forward(keep=...)`` and the trainer."""
        raise ValueError('the %s backward is not built: its backbone is run frozen, nothing is kept of its pass' % self.title)


class DeepLabBackbone(Backbone):
    """units and filters: the bottleneck groups of the DeepLab-ResNet.  7x7 s2 conv, max-pool (ssc_max_pool3s2), bottleneck units
    -- hip.conv_forward with the producer's frozen norm and relu folded into the consumer's View, ssc_residual_merge at every unit's
    end.  Groups 4 and 5 (atrous rates 2 and 4) run in the space-to-batch layout, where their 3x3 convs are plain ones:
    ssc_space_to_batch(2) in front of either group, ssc_batch_to_space(2) twice behind the last unit."""
    name, title, scope, model_name = 'deeplab', 'DeepLab-ResNet', 'ResNet/', 'deeplab_RMI'
    released = (64, 256, 512, 1024, 2048)
    size_reason = 'its 1/8 map is cut into 4 x 4 sub-images'
    trainable = True
    CONV1, CONV1_NORM = scope + 'group_1/conv1/DW', scope + 'group_1/bn_conv1'

    def widths(self):
        """A bottleneck's inner width is a quarter of its outer one."""
        return [('filters[0]', self.filters[0])] + [('filters[%d] / 4' % k, f // 4) for k, f in enumerate(self.filters) if k]

    @property
    def feat_channels(self):
        """The channels of the visual feature map: the last group's."""
        return self.filters[4]

    def unit_list(self):
        """[(scope, cin, cout, stride, rate)] of the bottleneck units in order."""
        out, f = [], self.filters
        for g, (n, stride, rate) in enumerate(zip(self.units, (1, 2, 1, 1), (1, 1, 2, 4))):
            for i in range(n):
                out.append(('%sgroup_%d_%d' % (self.scope, g + 2, i), f[g] if i == 0 else f[g + 1], f[g + 1], stride if i == 0 else 1, rate))
        return out

    def variable_shapes(self):
        """{checkpoint name: shape} of the backbone's variables, in the order every recorded digest depends on."""
        s, f = {}, self.filters

        def norm(scope, c):
            for p in NORM_PARTS:
                s[scope + '/' + p] = (1,) if p == 'factor' else (c,)
        s[self.CONV1] = (7, 7, 3, f[0])
        norm(self.CONV1_NORM, f[0])
        for scope, cin, cout, _stride, _rate in self.unit_list():
            c4 = cout // 4
            for blk, shape in (('block_1', (1, 1, cin, c4)), ('block_2', (3, 3, c4, c4)), ('block_3', (1, 1, c4, cout))) + \
                    ((('block_add', (1, 1, cin, cout)),) if cin != cout else ()):
                s['%s/%s/conv/DW' % (scope, blk)] = shape
                norm('%s/%s/bn' % (scope, blk), shape[3])
        return s

    def device_tensors(self, host=None):
        """What the kernels read, in the order of MatchModel.flat: the filters as stored, every norm as its [a | b] table under
        its scope.  host None: {device name: shape}; host {checkpoint name: array}: {device name: array}."""
        out = {}
        for name, shape in self.variable_shapes().items():
            scope, leaf = name.rsplit('/', 1)
            if leaf == 'DW':
                out[name] = shape if host is None else host[name]
            elif leaf == 'gamma':
                out[scope] = (2 * shape[0],) if host is None else fold_norm(*[host[scope + '/' + p] for p in NORM_PARTS])
        return out

    def trained_variable_names(self):
        """The filters: the norms stay as they were loaded."""
        return [n for n in self.variable_shapes() if n.endswith('/DW')]

    # ------------------------------------------------------------------ the pass on a MatchModel's buffers (m._buf) and weights (m.d)
    # Every pass below takes ``keep``.  None: inference -- the intermediate buffers are shared from unit to unit, nothing beyond
    # the result outlives the pass.  A dict: training -- every output the backward reads goes to a buffer of its own (bt/*), and
    # the dict is filled with the record the backward reads (match_backbone_train.py).  The launches and their operands' values
    # are the same either way.
    def unit(self, m, x, scope, stride, slot=0, keep=None):
        """One bottleneck unit on x float [N,H,W,cin] (materialised) -> relu(norm(block_3) + shortcut) [N,H/stride,W/stride,cout].
        Each raw conv output is read by its consumer through the producer's folded norm and relu.  keep: x, r1, r2, r3, sc (None
        for the identity shortcut) and out, in buffers bt/<scope>/*."""
        from . import hip
        from .hip import ACT_RELU, View
        d = m.d
        n, h, w, cin = x.shape
        oh, ow = -(-h // stride), -(-w // stride)
        w1, w2, w3 = (d['%s/block_%d/conv/DW' % (scope, k)] for k in (1, 2, 3))
        c4, cout = w1.shape[3], w3.shape[3]
        # inference: the units share r1, r2, r3 and sc, and alternate between two outputs (a unit reads its predecessor's)
        own, out_tag = ('', 'out%d' % slot) if keep is None else ('bt/%s/' % scope, 'bt/%s/out' % scope)
        r1 = m._buf(own + 'r1', (n, oh, ow, c4))
        hip.conv_forward(View(x), w1, stride, 0, r1, same=True)
        r2 = m._buf(own + 'r2', (n, oh, ow, c4))
        hip.conv_forward(View(r1, None, d[scope + '/block_1/bn'], ACT_RELU), w2, 1, 0, r2, same=True)
        r3 = m._buf(own + 'r3', (n, oh, ow, cout))
        hip.conv_forward(View(r2, None, d[scope + '/block_2/bn'], ACT_RELU), w3, 1, 0, r3, same=True)
        out = m._buf(out_tag, (n, oh, ow, cout))
        assert out.data_ptr() != x.data_ptr()
        wadd = d.get(scope + '/block_add/conv/DW')
        sc = None
        if wadd is not None:
            sc = m._buf(own + 'sc', (n, oh, ow, cout))
            hip.conv_forward(View(x), wadd, stride, 0, sc, same=True)
        else:
            assert cin == cout and stride == 1, (scope, cin, cout, stride)
        hip.call('ssc_residual_merge', r3, d[scope + '/block_3/bn'], x if sc is None else sc, d.get(scope + '/block_add/bn'), ACT_RELU,
                 out, n * oh * ow, cout)
        if keep is not None:
            keep.update(scope=scope, stride=stride, x=x, r1=r1, r2=r2, r3=r3, sc=sc, out=out)
        return out

    def regroup(self, m, x, rate_from, rate_to, tag='s2b'):
        """x in the space-to-batch layout of rate_from (1: the image itself) -> the layout of rate_to (2 or 4), in the buffer
        ``tag``: one ssc_space_to_batch(2).  Applied to the rate-2 layout it leaves sub-image (n*4 + i1*2 + j1)*4 + i2*2 + j2 with
        the pixels y % 4 == 2*i2 + i1, x % 4 == 2*j2 + j1: every sub-image is one residue class mod 4, which is all a rate-4 conv
        asks."""
        from . import hip
        assert rate_to == 2 * rate_from, (rate_from, rate_to)
        n, h, w, c = x.shape
        return hip.space_to_batch(x, 2, out=m._buf(tag, (n * 4, h // 2, w // 2, c)))

    def ungroup(self, m, x, rate, tag='b2s'):
        """The way back from ``regroup``: one ssc_batch_to_space(2) per halving of the rate, into the buffer ``tag`` formatted
        with the rate it arrives at."""
        from . import hip
        while rate > 1:
            nb, h, w, c = x.shape
            rate //= 2
            x = hip.batch_to_space(x, 2, out=m._buf(tag.format(rate), (nb // 4, h * 2, w * 2, c)))
        return x

    def forward(self, m, x4, keep=None):
        """x4 float [1,S,S,4] (ssc_match_preprocess_u8) -> the visual feature [1,S/8,S/8,filters[4]].  keep: x4, r0 (conv1's raw
        output) and units, the list of every unit's record with ``regroups``, the space_to_batch(2) moves in front of it; the
        buffers are those of match_backbone_train.forward_buffer_shapes."""
        from . import hip
        from .hip import View
        d, s = m.d, self.size
        own = '' if keep is None else 'bt/'
        r0 = m._buf(own + 'conv1', (1, s // 2, s // 2, self.filters[0]))
        hip.conv_forward(View(x4), d[self.CONV1], 2, 0, r0, same=True)
        x = hip.max_pool3s2(r0, d[self.CONV1_NORM], out=m._buf(own + 'pool', (1, s // 4, s // 4, self.filters[0])))
        cur, units = 1, []
        for k, (scope, _cin, _cout, stride, rate) in enumerate(self.unit_list()):
            rec = None if keep is None else {'regroups': 0}
            while cur < rate:
                x = self.regroup(m, x, cur, cur * 2, 's2b' if keep is None else 'bt/s2b%d' % (cur * 2))
                cur *= 2
                if rec is not None:
                    rec['regroups'] += 1
            x = self.unit(m, x, scope, stride, k & 1, keep=rec)
            units.append(rec)
        if keep is not None:
            keep.update(units=units, x4=x4, r0=r0)
        return self.ungroup(m, x, cur, 'b2s' if keep is None else 'bt/b2s{}')     # group_last's relu: the last unit's output is one already


class SegNetBackbone(Backbone):
    """filters: the widths of enc_1 .. enc_5 of segnet_model.py, units is not read.  18 3x3 convs, each behind the batch-statistics
    norm of the one image, five 2x2 pools that remember where each maximum was (ssc_max_pool2_argmax) and two unpools that put
    values back there (ssc_unpool2)."""
    name, title, scope, model_name = 'segnet', 'SegNet', 'SegNet/', 'segnet_RMI'
    released = (64, 128, 256, 512, 512)
    size_reason = 'SegNet pools 2 x 2 five times'
    ONES = scope + 'ones'       # the scale of a norm without gamma

    def widths(self):
        """The convs have the widths themselves."""
        return [('filters[%d]' % k, f) for k, f in enumerate(self.filters)]

    @property
    def feat_channels(self):
        """The channels of the visual feature map: dec_4's (= enc_4's)."""
        return self.filters[3]

    def stages(self):
        """[(stage, [(cin, cout)] of its 3x3 convs)] of segnet_model.py:56-95 up to intermediate_feat.  An encoder stage ends in
        its 2x2 pool; a decoder stage begins with the unpool by the codes of the encoder stage of its number, whose width its
        input therefore has: dec_5 ends at enc_4's width."""
        f1, f2, f3, f4, f5 = self.filters
        return [('enc_1', [(3, f1), (f1, f1)]), ('enc_2', [(f1, f2), (f2, f2)]), ('enc_3', [(f2, f3), (f3, f3), (f3, f3)]),
                ('enc_4', [(f3, f4), (f4, f4), (f4, f4)]), ('enc_5', [(f4, f5), (f5, f5), (f5, f5)]),
                ('dec_5', [(f5, f5), (f5, f5), (f5, f4)]), ('dec_4', [(f4, f4), (f4, f4)])]

    def plan(self):
        """The device pass as [(op, stage, k, channels in, channels out, side in, side out)], op one of 'conv' (k: the conv's
        number from 0), 'pool', 'act' (a decoder stage's last norm and relu materialised) and 'unpool'."""
        plan, h = [], self.size
        for stage, convs in self.stages():
            if stage.startswith('dec'):
                plan.append(('unpool', stage, None, convs[0][0], convs[0][0], h, 2 * h))
                h *= 2
            for k, (cin, cout) in enumerate(convs):
                plan.append(('conv', stage, k, cin, cout, h, h))
            if stage.startswith('enc'):
                plan.append(('pool', stage, None, cout, cout, h, h // 2))
                h //= 2
            else:
                plan.append(('act', stage, None, cout, cout, h, h))
        return plan

    def scratch_floats(self):
        """The floats of the two scratch buffers the pass alternates between: every step reads what the step before it wrote and
        writes into the other buffer, so each holds the largest tensor that falls to it; the last step's output (the feature map)
        has a buffer of its own."""
        need = [0, 0]
        for n, (_op, _stage, _k, _cin, cout, _h, oh) in enumerate(self.plan()[:-1]):
            need[n & 1] = max(need[n & 1], oh * oh * cout)
        return need

    def scratch_bytes(self):
        """The two scratch buffers, the input, the codes of the five pools (one byte per pooled element) and the feature map."""
        codes = sum(oh * oh * cout for op, _s, _k, _cin, cout, _h, oh in self.plan() if op == 'pool')
        return 4 * (sum(self.scratch_floats()) + self.size * self.size * 4 + (self.size // 8) ** 2 * self.feat_channels) + codes

    def norm_scope(self, stage, k):
        """The scope of the norm behind conv k (from 0) of a stage: tf.contrib.layers.batch_norm's default scope, numbered within
        the stage in call order -- BatchNorm, BatchNorm_1, BatchNorm_2."""
        return '%s%s/BatchNorm%s' % (self.scope, stage, '' if k == 0 else '_%d' % k)

    def variable_shapes(self):
        """{checkpoint name: shape} of the backbone's variables, the moving moments that ride along unread included, in the order
        every recorded digest depends on."""
        s = {}
        for stage, convs in self.stages():
            for k, (cin, cout) in enumerate(convs):
                s['%s%s/conv%d/DW' % (self.scope, stage, k + 1)] = (3, 3, cin, cout)
                s['%s%s/conv%d/biases' % (self.scope, stage, k + 1)] = (cout,)
            for k, (_cin, cout) in enumerate(convs):        # the norms of a stage are numbered in call order
                for p in SEGNET_NORM_PARTS:
                    s['%s/%s' % (self.norm_scope(stage, k), p)] = (cout,)
        return s

    def missing_variable(self, name, shape):
        """A checkpoint without the moving moments: their initial values; nothing reads them, snapshots carry them."""
        if name.rsplit('/', 1)[1] in SEGNET_NORM_PARTS[1:]:
            return (np.ones if name.endswith('variance') else np.zeros)(shape, dtype=np.float32)
        return None

    def device_tensors(self, host=None):
        """What the kernels read, in the order of MatchModel.flat: the filters (the first one's 3 input channels padded to 4), the
        betas and ``ONES``; the biases cancel in the norm and the moving moments are never read.
        host None: {device name: shape}; host {checkpoint name: array}: {device name: array}."""
        out = {}
        for name, shape in self.variable_shapes().items():
            leaf = name.rsplit('/', 1)[1]
            if leaf == 'DW':
                pad = max(4 - shape[2], 0)
                out[name] = (3, 3, shape[2] + pad, shape[3]) if host is None else np.pad(host[name], ((0, 0), (0, 0), (0, pad), (0, 0)))
            elif leaf == 'beta':
                out[name] = shape if host is None else host[name]
        out[self.ONES] = (max(self.filters),) if host is None else np.ones(max(self.filters), np.float32)
        return out

    def forward(self, m, x4, keep=None):
        """segnet_model.py:56-99, is_intermediate: x4 float [1,S,S,4] -> the visual feature [1,S/8,S/8,filters[3]] in the buffer
        sn/feat.  Every conv is followed by the batch-statistics norm of its one image (no gamma, eps 0.001) and a relu:
        hip.conv_forward folds the statistics to [a | b] behind the conv, and the next conv or the pool applies them and the relu
        as it loads.  The conv's bias is left out: the norm takes it off again with the mean.  The steps alternate between two
        scratch buffers (``scratch_floats``); the pools' codes have buffers of their own (sn/code/<stage>), enc_5's and enc_4's
        are read by the unpools.  keep: refused."""
        if keep is not None:
            self.trained_variable_names()
        import torch
        from . import hip
        from .hip import ACT_NONE, ACT_RELU, View
        d = m.d
        plan = self.plan()
        flat = [m._buf('sn/scratch%d' % k, (n,)) for k, n in enumerate(self.scratch_floats())]
        x, ab, codes = x4, None, {}
        for n, (op, stage, k, cin, cout, h, oh) in enumerate(plan):
            last = n == len(plan) - 1
            out = m._buf('sn/feat', (1, oh, oh, cout)) if last else flat[n & 1][:oh * oh * cout].view(1, oh, oh, cout)
            assert out.data_ptr() != x.data_ptr()
            if op == 'conv':
                norm = self.norm_scope(stage, k)
                ab_new, stats = m._buf('sn/ab/' + norm, (2 * cout,)), m._buf('sn/stats/' + norm, (2 * cout,))
                hip.conv_forward(View(x, None, ab, ACT_RELU if ab is not None else ACT_NONE),
                                 d['%s%s/conv%d/DW' % (self.scope, stage, k + 1)], 1, 0, out, same=True,
                                 bn=(d[self.ONES][:cout], d[norm + '/beta'], ab_new, stats, NORM_EPS))
                ab = ab_new
            elif op == 'pool':
                codes[stage] = m._buf('sn/code/' + stage, (1, oh, oh, cout), torch.uint8)
                hip.max_pool2_argmax(x, ab, out=out, code=codes[stage])
                ab = None
            elif op == 'act':       # a decoder stage's last norm and relu, materialised for the unpool and for the head
                hip.call('ssc_affine_act', x, cout, ab, cout, ACT_RELU, out, cout, oh * oh, cout)
                ab = None
            else:
                hip.unpool2(x, codes['enc_' + stage[4:]], out=out)
            x = out
        return x


BACKBONES = {b.name: b for b in (DeepLabBackbone, SegNetBackbone)}
