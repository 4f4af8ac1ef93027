"""Pieces the Pix2Pix, Residual and MRU networks share: the row view of an NHWC tensor, the per-pass gradient slots of the
tape-driven backward passes, and the spectral-normed auxiliary classifier on the spatial mean of a late layer
(fully_connected/weights [C, K] under sn.py; models_collection.py:789-841, 844-893, 676-786)."""
from . import hip

FC = 'discriminator/fully_connected/'


def _rows(t):
    return t if t.dim() == 2 else t.view(-1, t.shape[-1])


class GradSlots(object):
    """Gradient buffers of one backward pass, keyed by the address of the tensor they belong to (``self._gdone``, reset by the
    pass; ``self.b``: the Buffers)."""

    _gtag = ''

    def _gslot(self, t):
        """Gradient buffer of tensor ``t`` for this backward pass: (buffer, accumulate?)."""
        key = t.data_ptr()
        if key in self._gdone:
            return self._gdone[key], True
        # (_gtag: two backward passes through ONE forward context that run on different streams -- BGTrainer's fake pair -- must
        # not share these buffers: the pass names its set)
        g = self.b.get('grad_of/%s%d' % (self._gtag, key), t.shape)
        self._gdone[key] = g
        return g, False

    def _gget(self, t):
        return self._gdone.get(t.data_ptr())


def class_head_forward(store, bufs, tag, x, wbar):
    """logits [N, K] = x [N, C] @ wbar + biases."""
    N, C = x.shape
    K = store[FC + 'weights'].shape[1]
    logits = bufs.get(tag + '/logits', (N, K))
    hip.call('ssc_fc_small_fwd', x, wbar, store[FC + 'biases'], N, C, K, logits)
    return logits


def class_head_backward(store, x, st, dlogits, dx, need_params, sn=True, accumulate=False):
    """dx [N, C] = d loss / d x; with need_params the bias gradient and the gradient w.r.t. the weights the forward multiplied
    with: W_bar under spectral norm (``st['gwbar']``, summed over the calls of this step: ``st['n_acc']``), W itself otherwise
    (written, or added with ``accumulate``).  st: the spectral-norm state of fully_connected/weights."""
    N, C = x.shape
    gw, gb_, acc = None, None, 0
    if need_params:
        gb_ = store.grad(FC + 'biases')
        if sn:
            gw, acc = st['gwbar'], int(st['n_acc'] > 0)
            st['n_acc'] += 1
        else:
            gw, acc = store.grad(FC + 'weights'), int(accumulate)
    hip.call('ssc_fc_small_bwd', x, st['wbar'], dlogits, N, C, dlogits.shape[1], dx, gw, gb_, acc)
    return dx


class SnClassHead(object):
    """The class head of the Pix2Pix and Residual discriminators (``self.s``, ``self.b``, ``self.sn``): one spectral-normed
    weight, one power iteration per step."""

    def prepare_sn(self, tag='d/sn', u=None):
        """One power iteration on fully_connected/weights (sn.py), shared by every call of this step.
        tag / u: buffers and starting vector of a pass that runs beside another step's (the discriminator's real pass run
        ahead inside the generator step starts from the u that step is about to assign: trainer._d_real_pass)."""
        s, B = self.s, self.b
        W = s[FC + 'weights']
        m, n = W.shape
        if not self.sn:
            return {'wbar': W}
        sn = {'v': B.get(tag + '/v', (m,)), 'u_new': B.get(tag + '/u_new', (1, n)), 'wbar': B.get(tag + '/wbar', (m, n)),
              'aux': B.get(tag + '/aux', (4,)), 'gwbar': B.get(tag + '/gwbar', (m, n)), 'n_acc': 0,
              'scratch': B.get(tag + '/scratch', (m,)), 'u': (u if u is not None else s[FC + 'u'])}
        hip.call('ssc_sn_forward', W, sn['u'], m, n, sn['v'], sn['u_new'], sn['wbar'], sn['aux'])
        return sn

    def _head_forward(self, tag, img, sn):
        return class_head_forward(self.s, self.b, tag, img, sn['wbar'])

    def _head_backward(self, ctx, sn, dlogits, need_params, accumulate):
        """Returns dimg [N, 512], the gradient w.r.t. the spatial mean the head read (ctx['img'])."""
        dimg = self.b.get(ctx['tag'] + '/gb/dimg', ctx['img'].shape)
        return class_head_backward(self.s, ctx['img'], sn, dlogits, dimg, need_params, self.sn, accumulate)

    def finish_sn_backward(self, sn, accumulate=False):
        """d loss / d W from the accumulated d loss / d W_bar, through sigma and the power iteration."""
        s = self.s
        if not self.sn:
            return
        W = s[FC + 'weights']
        m, n = W.shape
        gW = s.grad(FC + 'weights')
        if sn['n_acc'] == 0:
            if not accumulate:
                hip.fill(gW, 0.0)
            return
        hip.call('ssc_sn_backward', W, sn['u'], sn['v'], sn['u_new'], sn['aux'], sn['gwbar'], m, n, gW, int(accumulate),
                 sn['scratch'])
