"""Background_Colorization module (bg_colorization_main.py:302-726): the generator behind the reference's function name and
the whole train step.

``create_residual_generator`` is the forward pass (BASELINE.json config 5, the 768x768 large-activation stress case).  The
reference builds the variables under tf.variable_scope('generator') (:582-586); they live in a ``ParamStore('BG')`` keyed by
those TF names so a converted checkpoint loads with ``store.load_dict``.

``BGTrainer`` is ``create_model`` in train mode: generator with region branch, residual discriminator, the three loss terms,
Adam(beta1 = 0.5) with the polynomial step size, one ``sess.run(model.train)`` per ``train_step``, replayed from a hipGraph.
``train_step`` takes float images; ``train_step_u8`` takes the loader's uint8 arrays and makes the float images, the
discriminator's real pair and the masked-L1 pixel count from them in one launch inside the graph (csrc/bg_io.hip);
``train_step_cached`` takes the entries of scenes that a ``scene_cache.SceneCache`` keeps on the device and gathers them in that
launch, with the labels and an optional sky / ground recolouring.  All take
any batch N: the reference's placeholders are fixed at 1 (:765-768), nothing else in its graph is, and at N > 1 the norms'
statistics, the loss means and the masked-L1 count run over the whole batch -- what the float64 oracle computes
(tests/test_gpu_residual.py holds the trainer to it at N = 2).  The command line (bg_colorization_main.py of this repository)
drives ``train_step_u8`` at ``--batch_size N`` and writes test-mode PNGs through ``hip.bg_finish_u8``.
"""
import contextlib
import numpy as np
import os

import torch

from . import hip
from .params import Buffers, ParamStore
from .pinned_ring import PinnedRing
from .residual import ResidualGenerator
from .step_graphs import FAILED, StepGraphs

_TOWERS = {}
MASK_CLASSES = 3        # data_processing.image_processing.load_region_mask writes the classes 0, 1, 2


def check_seg_classes(seg_classes):
    """The region-mask loss indexes a row of ``seg_classes`` logits with the mask's label (tf.nn.sparse_softmax_cross_entropy_
    with_logits raises -- on a GPU: answers NaN -- for a label outside them).  The masks carry classes 0 .. 2 and the kernel
    holds at most four logits per row, so a trainer for fewer or more classes is refused where it is built; a label that is
    out of range all the same (a mask from elsewhere) makes ssc_seg_ce_loss answer NaN instead of reading past the row."""
    if not MASK_CLASSES <= int(seg_classes) <= 4:
        raise ValueError('seg_classes = %s: the region masks carry the classes 0 .. %d and the loss kernel takes at most 4 '
                         'logits per pixel, so seg_classes must be %d or 4' % (seg_classes, MASK_CLASSES - 1, MASK_CLASSES))


def get_tower(image_size=768, vocab_size=18, ngf=64, seg_classes=3, seed=0, device='cuda'):
    key = (image_size, vocab_size, ngf, seg_classes)
    if key not in _TOWERS:
        if ngf != 64:
            raise NotImplementedError('ngf=%d: the parameter registry is laid out for the default ngf=64' % ngf)
        hip.lib()
        store = ParamStore('BG', vocab_size, image_size, device, seed)
        bufs = Buffers(device)
        _TOWERS[key] = (store, bufs, ResidualGenerator(store, bufs, 'bg', True, ngf, seg_classes))
    return _TOWERS[key]


def reset():
    _TOWERS.clear()


def create_residual_generator(generator_inputs, generator_outputs_channels, vocab_indices, ngf=64, vocab_size=18,
                              seg_classes=3, multi_residual=True):
    """generator_inputs NHWC [N,H,W,3] in [-1,1], vocab_indices int [N,T] ->
    (outputs NHWC [N,H,W,3] = tanh image, region_mask_logits NHWC [N,H,W,seg_classes])."""
    if not multi_residual or generator_outputs_channels != 3:
        raise NotImplementedError('only multi_residual=True, 3 output channels (the reference defaults, :805-807)')
    x = torch.as_tensor(np.asarray(generator_inputs) if not isinstance(generator_inputs, torch.Tensor)
                        else generator_inputs).to(device='cuda', dtype=torch.float32).contiguous()
    text = vocab_indices.cpu().numpy() if isinstance(vocab_indices, torch.Tensor) else np.asarray(vocab_indices)
    store, bufs, gen = get_tower(x.shape[1], vocab_size, ngf, seg_classes)
    ctx = gen.forward(x, text, None, 'bg')
    return ctx['image'], ctx['region_logits']


# ---------------------------------------------------------------------------------------------------------------
# training (create_model in train mode, bg_colorization_main.py:516-726)
# ---------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _beside(side):
    """The block is issued on the stream ``side``, behind what the current stream holds so far -- or in line when ``side`` is
    None.  The caller joins: ``main.wait_stream(side)`` where the block's results are read."""
    if side is not None:
        side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):       # (of None: the current stream stays)
        yield


class BGTrainer(object):
    """Generator + residual discriminator of the BG module with the reference's losses and optimizer:

        discrim_loss = mean(-(log(D(x, y) + eps) + log(1 - D(x, G(x)) + eps)))
        gen_loss     = gan_weight * mean(-log(D(x, G(x)) + eps)) + l1_weight * mean_{label != 0} |y - G(x)|
                       + seg_weight * mean CE(region logits, labels)
        Adam(lr_t, beta1 = 0.5, beta2 = 0.999) on both nets, lr_t = polynomial_decay(lr, step, 0.75 * max_steps,
        lr / 10, power 0.9).

    One ``train_step`` = one ``sess.run(model.train)`` (:898-901): a single forward pass, both gradient sets, both
    Adam applies.  The reference orders the generator's gradient ops after the discriminator update
    (control_dependencies, :648) without defining which discriminator weights they read; here both gradients are
    taken at the weights the forward pass used."""

    def __init__(self, image_size=768, vocab_size=18, ngf=64, ndf=64, seg_classes=3, lr=2e-4, max_steps=100000,
                 gan_weight=1.0, l1_weight=100.0, seg_weight=100.0, beta1=0.5, seed=0, device='cuda', use_graphs=True):
        check_seg_classes(seg_classes)
        if not torch.cuda.is_available():
            raise RuntimeError('BGTrainer needs an MI355X (HIP) device: there is no CPU fallback')
        if ngf != 64 or ndf != 64:
            raise NotImplementedError('the parameter registry is laid out for ngf = ndf = 64')
        from .residual import BGDiscriminator
        hip.lib()
        self.store = ParamStore('BG', vocab_size, image_size, device, seed)
        self.bufs = Buffers(device)
        self.G = ResidualGenerator(self.store, self.bufs, 'bg', True, ngf, seg_classes)
        self.D = BGDiscriminator(self.store, self.bufs, ndf)
        self.seg = seg_classes
        self.lr, self.max_steps = lr, max_steps
        self.w_gan, self.w_l1, self.w_seg = gan_weight, l1_weight, seg_weight
        self.beta1, self.beta2, self.eps = beta1, 0.999, 1e-8
        # [discrim_loss, gen_loss, gen_loss_GAN, gen_loss_L1, region_mask_loss] accumulated in double on the device
        self.losses = torch.zeros(5, dtype=torch.float64, device=device)
        for sc in (self.store.generator, self.store.discriminator):
            sc.adam_m = torch.zeros_like(sc.adam_v)
        self.global_step = 0
        # hipGraph replay of whole steps (as GanTrainer): ~1500 launches per step are otherwise issued one by one.  The
        # step sizes live in device memory so that one captured graph serves every step.
        self.use_graphs = bool(use_graphs)
        self.lr_dev = torch.zeros(2, dtype=torch.float32, device=device)
        self._step_graphs, self._static = StepGraphs(), {}
        self._graphs = self._step_graphs.graphs
        # D(real) -- forward, its loss term, backward into the discriminator's gradient buffer -- does not depend on the generator:
        # it runs on a stream of its own beside the generator forward, in the CUs that pass's many small launches leave idle
        # (SSC_BG_OVERLAP_REAL=0: everything in line, as rounds 3-5)
        self._real_stream = torch.cuda.Stream() if os.environ.get('SSC_BG_OVERLAP_REAL', '1') == '1' else None
        # (filter gradients on a stream of their own beside the data-gradient chain, hip.WGRAD_STREAM: measured 24.3-24.8 vs 22.5 ms,
        # same bits -- not kept; profiles/NOTEBOOK_r06.md section 6)

    def learning_rate(self, step):
        decay_steps = int(round(self.max_steps * 0.75))
        s = min(step, decay_steps)
        return (self.lr - self.lr / 10.0) * (1.0 - s / decay_steps) ** 0.9 + self.lr / 10.0

    def _pack(self, name, inputs, second):
        N, H, W, _ = inputs.shape
        xd = self.bufs.get(name, (N, H, W, 8), zero_on_alloc=True)
        M = N * H * W
        hip.call('ssc_strided_copy', inputs, 3, xd, 8, M, 3, 0)
        hip.call('ssc_strided_copy', second, 3, xd.view(-1)[3:], 8, M, 3, 0)
        return xd

    def gradients(self, inputs, targets, text, labels_gt, xd_real=None, count=None):
        """inputs / targets NHWC [N,H,W,3] in [-1,1], text int [N,T] (host), labels_gt int32 [N,H,W].
        Fills both flat gradient buffers and ``self.losses``; returns the generator context.
        xd_real [N,H,W,8] = the packed real pair [inputs | targets | 0 0] and count [1] = the number of labels != 0, when the
        caller has them already (``train_step_u8``: hip.bg_stage_u8 writes both); otherwise they are made here."""
        B = self.bufs
        inputs, targets = inputs.contiguous(), targets.contiguous()
        labels = labels_gt.to(device=inputs.device, dtype=torch.int32).contiguous()
        N, H, W, _ = inputs.shape
        M = N * H * W
        L = self.losses
        L.zero_()
        main = torch.cuda.current_stream()
        side = self._real_stream if hip.PROFILE is None else None      # per-kernel timing runs everything in line
        with _beside(side):     # D(real), beside the generator forward
            cr = self.D.forward(xd_real if xd_real is not None else self._pack('xd_real', inputs, targets), 'dr')
            nz = cr['z'].numel()
            dz_r = B.get('dz_r', cr['z'].shape)
            hip.call('ssc_bg_gan_loss', cr['z'], nz, 0, 1.0 / nz, L[0:1], dz_r, 1.0 / nz)
            self.D.backward(cr, dz_r, True, False, accumulate=False)
        gctx = self.G.forward(inputs, text, None, 'bg')
        image, logits = gctx['image'], gctx['region_logits']
        cf = self.D.forward(self._pack('xd_fake', inputs, image), 'df')
        ws = hip.workspace()
        # ---- discriminator loss and gradients (the fake term adds to the loss word and the gradient buffer the real pass wrote)
        if side is not None:
            main.wait_stream(side)
        dz_f = B.get('dz_f', cf['z'].shape)
        hip.call('ssc_bg_gan_loss', cf['z'], nz, 1, 1.0 / nz, L[0:1], dz_f, 1.0 / nz)
        # the fake pair's backward into the discriminator's gradient buffer is off the critical path (nothing reads it before
        # the optimizer): on the side stream, beside the generator's loss terms and backward pass.  The two passes through
        # the same forward context then need gradient scratch of their own: the generator's pass takes the 'dg' set.
        with _beside(side):
            self.D.backward(cf, dz_f, True, False, accumulate=True)
        cfg = cf if side is None else dict(cf, tag='dg', tape=[dict(rec, tag='dg') for rec in cf['tape']])
        # ---- generator loss and gradients
        dz_g = B.get('dz_g', cf['z'].shape)
        hip.call('ssc_bg_gan_loss', cf['z'], nz, 0, 1.0 / nz, L[2:3], dz_g, self.w_gan / nz)
        dgan = self.D.backward(cfg, dz_g, False, True, accumulate=False)
        if count is None:
            count = B.get('l1_count', (1,))
            hip.call('ssc_count_nonzero_i32', labels, M, count, ws, ws.numel() * 4)
        dpre = B.get('dpre', (N, H, W, 4))
        # (the kernel folds the weight into the gradient and writes every element of dpre)
        hip.call('ssc_bg_output_grad', image, targets, labels, count, float(self.w_l1), dgan, L[3:4], dpre, M)
        dlog = B.get('dlog', (N, H, W, 4), zero_on_alloc=True)
        hip.call('ssc_seg_ce_loss', logits, self.seg, labels, M, float(self.w_seg), L[4:5], dlog, 4)
        self.G.backward(gctx, dpre, None, dlogits=dlog)
        if side is not None:
            main.wait_stream(side)      # the discriminator's gradient buffer is complete
        return gctx

    def loss_values(self):
        """(discrim_loss, gen_loss, gen_loss_GAN, gen_loss_L1, region_mask_loss) as Python floats."""
        d, _, gan, l1w, segw = [float(v) for v in self.losses.tolist()]
        l1 = l1w / self.w_l1 if self.w_l1 else 0.0
        seg = segw / self.w_seg if self.w_seg else 0.0
        return d, gan * self.w_gan + l1w + segw, gan, l1, seg

    def _adam_prepare(self):
        """Host part of both Adam applies: advance t, put lr_t = lr*sqrt(1-b2^t)/(1-b1^t) in device memory."""
        lr = self.learning_rate(self.global_step)
        for i, sc in enumerate((self.store.discriminator, self.store.generator)):
            sc.adam_t += 1
            t = sc.adam_t
            self.lr_dev[i:i + 1].fill_(float(lr * (1.0 - self.beta2 ** t) ** 0.5 / (1.0 - self.beta1 ** t)))
        self.global_step += 1

    def _adam_launch(self):
        for i, sc in enumerate((self.store.discriminator, self.store.generator)):
            hip.call('ssc_adam_tf', sc.flat, sc.grad, sc.adam_m, sc.adam_v, sc.numel, 0.0, self.lr_dev[i:i + 1],
                     self.beta1, self.beta2, self.eps, 1.0)
            hip.refresh_splits(sc.flat)     # the bf16 planes of this scope's filters follow the weights

    def apply_gradients(self):
        self._adam_prepare()
        self._adam_launch()

    def train_step(self, inputs, targets, text, labels_gt):
        """One ``sess.run(model.train)``.  The first call of a shape runs eagerly (it allocates), the second is captured
        into a hipGraph, later ones replay it on the inputs copied into the graph's static tensors."""
        key = tuple(inputs.shape)
        st = self._statics(key, key)
        st['inputs'].copy_(inputs)
        st['targets'].copy_(targets)
        st['labels'].copy_(labels_gt)
        return self._run(key, st, text)

    def _statics(self, key, shape, extra=dict):
        """The static tensors of ``key``, made the first time it is seen: what every step reads -- the float ``inputs`` and
        ``targets`` [N,H,W,3] and the int32 ``labels`` [N,H,W] (zero until written) -- and what ``extra()`` adds for its caller."""
        if key not in self._static:
            dev = self.losses.device
            self._static[key] = dict(extra(), inputs=torch.empty(shape, dtype=torch.float32, device=dev),
                                     targets=torch.empty(shape, dtype=torch.float32, device=dev),
                                     labels=torch.zeros(shape[:3], dtype=torch.int32, device=dev))
        return self._static[key]

    def _run(self, key, st, text, stage=None):
        """One step on the static tensors ``st`` (inputs, targets, labels): filled by the caller, or made inside the step by the
        one launch ``stage(st, xd_real, count)``, which also writes the two arrays ``gradients`` then need not make.  Eager when
        graphs are off and under per-kernel timing; otherwise through ``_step``, one graph per ``key`` and live caption steps."""
        prep = text if isinstance(text, dict) else self.G.text.prepare(text, 'bg')

        def gradients():
            made = {}
            if stage is not None:
                made = {'xd_real': self.bufs.get('xd_real', tuple(st['inputs'].shape[:3]) + (8,), zero_on_alloc=True),
                        'count': self.bufs.get('l1_count', (1,))}
                stage(st, **made)
            return self.gradients(st['inputs'], st['targets'], prep, st['labels'], **made)

        if not self.use_graphs or hip.PROFILE is not None:
            gctx = gradients()
            self.apply_gradients()
            return gctx
        return self._step(key + (prep['S'],), gradients)

    def train_step_u8(self, fg_u8, bg_u8, text, labels):
        """``train_step`` fed with what the loader produces: fg_u8 / bg_u8 uint8 [N,H,W,3] (foreground = generator input,
        background = target), labels int32 [N,H,W]; host (best: pinned) or device tensors, or NumPy arrays.  They are copied
        into static tensors of the shape and one launch (hip.bg_stage_u8, inside the captured graph) makes the float images
        u8/255*2-1, the discriminator's packed real pair and the masked-L1 pixel count from them."""
        fg_u8, bg_u8, labels = [t if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t))
                                for t in (fg_u8, bg_u8, labels)]
        assert fg_u8.dtype == torch.uint8 and bg_u8.dtype == torch.uint8 and fg_u8.shape == bg_u8.shape
        assert fg_u8.dim() == 4 and fg_u8.shape[3] == 3 and tuple(labels.shape) == tuple(fg_u8.shape[:3]), \
            'labels %s for images %s' % (tuple(labels.shape), tuple(fg_u8.shape))
        dev, shape = self.losses.device, tuple(fg_u8.shape)
        key = ('u8',) + shape
        st = self._statics(key, shape, lambda: {'fg': torch.empty(shape, dtype=torch.uint8, device=dev),
                                                'bg': torch.empty(shape, dtype=torch.uint8, device=dev)})
        st['fg'].copy_(fg_u8, non_blocking=True)
        st['bg'].copy_(bg_u8, non_blocking=True)
        st['labels'].copy_(labels, non_blocking=True)
        return self._run(key, st, text, lambda st, xd_real, count: hip.bg_stage_u8(
            st['fg'], st['bg'], st['labels'], st['inputs'], st['targets'], xd_real, count))

    @staticmethod
    def _small_upload(st, name, values):
        """values (NumPy array or host tensor of the static tensor's shape) -> st[name], without a host wait: through the
        pinned ring st['ring_' + name], unless the values are on the device or pinned already."""
        if torch.is_tensor(values) and (values.is_cuda or values.is_pinned()):
            return st[name].copy_(values, non_blocking=True)
        buf = st['ring_' + name].next()
        buf.copy_(values if torch.is_tensor(values) else torch.from_numpy(np.ascontiguousarray(values, dtype=buf.numpy().dtype)))
        st[name].copy_(buf, non_blocking=True)
        st['ring_' + name].queued()

    def train_step_cached(self, cache, slots, recolor, text):
        """``train_step_u8`` on scenes that live on the device already: cache.fg / cache.bg uint8 [S,H,W,3] and cache.seg uint8
        [S,H,W] (the segment png's red channel; a ``scene_cache.SceneCache``), allocated once -- their addresses are part of the
        captured graph.  slots int [N,3] = the fg, bg and seg entry of each sample; recolor uint8 [N,8] = {enable, sky rgb,
        ground rgb, 0} per sample or None (nothing recoloured).  Only these two small arrays are copied in a step; one launch
        (hip.bg_stage_cached_u8, inside the graph) gathers the scenes and makes the float images, the labels, the packed real
        pair and the masked-L1 pixel count."""
        dev = self.losses.device
        assert cache.fg.device == dev and cache.fg.dtype == torch.uint8 and cache.fg.dim() == 4
        N, (H, W) = len(slots), cache.fg.shape[1:3]
        assert tuple(slots.shape) == (N, 3) and (recolor is None or tuple(recolor.shape) == (N, 8))
        key = ('cached', N, H, W, cache.fg.data_ptr(), cache.bg.data_ptr(), cache.seg.data_ptr(),
               cache.fg.shape[0], cache.bg.shape[0], cache.seg.shape[0])
        st = self._statics(key, (N, H, W, 3), lambda: {
            'slot': torch.zeros((N, 3), dtype=torch.int32, device=dev), 'ring_slot': PinnedRing((N, 3), torch.int32),
            'recolor': torch.zeros((N, 8), dtype=torch.uint8, device=dev), 'ring_recolor': PinnedRing((N, 8), torch.uint8),
            'painted': False})
        self._small_upload(st, 'slot', slots)
        if recolor is not None:
            self._small_upload(st, 'recolor', recolor)
            st['painted'] = True
        elif st['painted']:         # the static record still enables a colour pair of an earlier step
            st['recolor'].zero_()
            st['painted'] = False
        return self._run(key, st, text, lambda st, xd_real, count: hip.bg_stage_cached_u8(
            cache.fg, cache.bg, cache.seg, st['slot'], st['recolor'], st['inputs'], st['targets'], xd_real, st['labels'], count))

    def _step(self, key, gradients):
        """The optimizer step around ``gradients()`` (which reads static tensors only), eager the first time ``key`` is seen,
        captured the second time, replayed from then on."""
        self._adam_prepare()

        def impl():
            self._gctx = gradients()
            self._adam_launch()

        outcome, _ = self._step_graphs.run(key, impl, (self.store.discriminator.flat, self.store.generator.flat))
        if outcome == FAILED:       # never lose a training run to graph capture: eager launches from here on
            self.use_graphs = False
            torch.cuda.synchronize()
            if self._real_stream is not None:       # it forked inside the abandoned capture: not used again
                self._real_stream = torch.cuda.Stream()
            impl()
        return self._gctx

    def color_foreground(self, fg_u8, tok):
        """Test mode's forward pass: fg_u8 uint8 [1,H,W,3] on the device and its token row int [1,T] (host) -> the generator
        context of ``G.forward`` on u8 / 255 * 2 - 1 (``['image']``: the tanh image, valid until the next pass under tag 'bg').
        One image, whatever the batch of training: the norms are batch statistics."""
        shape, dev = tuple(fg_u8.shape), fg_u8.device
        st = self._statics(('fg',) + shape, shape, lambda: {'xd': torch.empty(shape[:3] + (8,), dtype=torch.float32, device=dev),
                                                            'count': torch.empty(1, device=dev)})
        # the forward pass reads the stage's float inputs only: the foreground stands in for the background and the constant zero
        # labels, so nothing but the foreground is uploaded (targets, xd and count are the kernel's other outputs, unread)
        hip.bg_stage_u8(fg_u8, fg_u8, st['labels'], st['inputs'], st['targets'], st['xd'], st['count'])
        return self.G.forward(st['inputs'], tok, None, 'bg')
