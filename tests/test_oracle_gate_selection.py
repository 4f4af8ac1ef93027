"""oracle.mru.gate_selection: the optional selection of the min-max gates' extremal positions (CPU only)."""
import torch

from oracle import mru as M


def _plane(values):
    return torch.tensor(values, dtype=torch.float64).view(1, 1, 1, -1)


def test_no_selection_keeps_the_plain_gate_bit_for_bit():
    x = torch.randn(2, 3, 5, 4, generator=torch.Generator().manual_seed(0))
    want = (x - x.amin(dim=(2, 3), keepdim=True)) / (x.amax(dim=(2, 3), keepdim=True) - x.amin(dim=(2, 3), keepdim=True))
    assert torch.equal(M._minmax(x), want) and torch.equal(M._minmax(x, 'a/gate'), want)
    rec = {}
    with M.gate_selection({}, record=rec):
        assert torch.equal(M._minmax(x, 'a/gate'), want)
    assert list(rec) == [(None, 'a/gate')] and torch.equal(rec[(None, 'a/gate')], x)
    assert M._GATE_CTX is None


def test_tied_selection_is_the_reduce_min_max_gradient():
    """All tied positions selected: value and gradient of amin / amax (which divide evenly over ties, as TensorFlow does)."""
    x = _plane([1, 0, 0, 3, 3, 3, 2]).requires_grad_(True)
    w = _plane([0.3, -1.0, 2.0, 0.5, 0.7, -0.2, 1.1])
    (M._minmax(x) * w).sum().backward()
    want = x.grad.clone()
    x.grad = None
    xd = x.detach()
    with M.gate_selection({(None, 'g'): (xd == xd.min(), xd == xd.max())}):
        r = M._minmax(x, 'g')
    assert torch.equal(r.detach(), M._minmax(xd))
    (r * w).sum().backward()
    assert torch.allclose(x.grad, want, rtol=0, atol=1e-15)


def test_near_tie_selection_moves_the_gradient_to_the_selected_position():
    """Position 2 is 1e-9 above the minimum at position 1: selecting it moves the gate by that gap and sends the whole
    reduce_min gradient there."""
    vals = [1.0, 0.0, 1e-9, 3.0, 2.0]
    x = _plane(vals).requires_grad_(True)
    w = _plane([0.3, -1.0, 2.0, 0.5, 0.7])
    (M._minmax(x) * w).sum().backward()
    plain = x.grad.clone()
    x.grad = None
    sel_min = torch.tensor([False, False, True, False, False]).view(1, 1, 1, -1)
    sel_max = torch.tensor([False, False, False, True, False]).view(1, 1, 1, -1)
    with M.gate_selection({(None, 'g'): (sel_min, sel_max)}):
        r = M._minmax(x, 'g')
    assert float((r.detach() - M._minmax(x.detach())).abs().max()) < 1e-9
    (r * w).sum().backward()
    moved = x.grad
    through_min = plain[0, 0, 0, 1] - w[0, 0, 0, 1] / 3.0        # what reduce_min received, without the position's own term
    assert abs(float(moved[0, 0, 0, 2] - plain[0, 0, 0, 2] - through_min)) < 1e-8
    assert abs(float(moved[0, 0, 0, 1] - w[0, 0, 0, 1] / 3.0)) < 1e-8
    assert torch.allclose(moved[0, 0, 0, [0, 3, 4]], plain[0, 0, 0, [0, 3, 4]], rtol=0, atol=1e-8)


def test_training_graph_names_its_22_gates_and_exact_selection_changes_nothing():
    from oracle import pix2pix as O
    p = M.init_params(0, with_discriminator=True, img=32)
    b = O.synthetic_batch(1, seed=3, img=32)
    rec = {}
    with M.gate_selection({}, record=rec):          # (an empty selection: the plain graph, see the first test)
        plain = M.build_single_graph_f64(p, **b)
    assert sorted(k[0] for k in rec) == ['d_fake'] * 4 + ['d_real'] * 4 + ['generator'] * 14
    assert ('generator', 'generator/mru_deconv_unit_t_8_layer_0/Conv_1') in rec
    assert ('d_real', 'discriminator/mru_conv_unit_t_4_layer_0/update_gate') in rec
    sel = {k: (v == v.amin(dim=(2, 3), keepdim=True), v == v.amax(dim=(2, 3), keepdim=True)) for k, v in rec.items()}
    with M.gate_selection(sel):
        r = M.build_single_graph_f64(p, **b)
    for s in ('grad_g', 'grad_d'):
        for k, g in plain[s].items():
            assert float((r[s][k] - g).norm()) <= 1e-12 * max(float(g.norm()), 1e-30), k
    assert float(r['loss_g']) == float(plain['loss_g']) and float(r['loss_d']) == float(plain['loss_d'])
