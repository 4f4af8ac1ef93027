"""Golden fixtures: caption->indices from the real reference module; frozen oracle outputs."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import pix2pix as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def test_text_processing_matches_reference_goldens():
    from sketchyscenecolorization_amd.data_processing import text_processing as tp
    g = json.load(open(os.path.join(GOLD, 'text_goldens.json')))
    from sketchyscenecolorization_amd.data_processing.default_vocab import default_vocab_dict
    pkg_vocab = default_vocab_dict()
    assert pkg_vocab == g['vocab'] and len(pkg_vocab) == 58 and pkg_vocab['<pad>'] == 0 and pkg_vocab['<unk>'] == 1
    for case in g['cases']:
        assert tp.preprocess_sentence(case['sentence'], g['vocab'], g['T']) == case['indices'], case['sentence']
    for case in g['cases_T8']:
        assert tp.preprocess_sentence(case['sentence'], g['vocab'], 8) == case['indices']
    # SURVEY 8c known answers
    assert tp.preprocess_sentence('the car is yellow with blue window', g['vocab'], 15) == [0] * 9 + [28, 3, 16, 22, 15, 1]


def _load():
    z = np.load(os.path.join(GOLD, 'pix2pix_img64_n2_seed0_42.npz'))
    p = O.init_params(0, img=64)
    b = O.synthetic_batch(2, seed=42, img=64)
    return z, p, b


def test_oracle_reproduces_frozen_outputs():
    z, p, b = _load()
    gen = O.generate_pix2pix(p, b['sketches'], b['text'], b['noise_vec']).numpy()
    assert np.abs(gen - z['gen']).max() < 2e-5
    r = O.build_single_graph_f64(p, **b)
    assert abs(float(r['loss_g']) - float(z['loss_g'])) < 1e-9 and abs(float(r['loss_d']) - float(z['loss_d'])) < 1e-9
    for k in z.files:
        if k.startswith('l2_'):
            name = k[3:].replace('.', '/')
            g = r['grad_g' if name.startswith('gen') else 'grad_d'][name]
            assert abs(float(g.norm()) - float(z[k])) < 1e-9 * max(1.0, float(z[k]))


@pytest.mark.gpu
def test_hip_matches_frozen_outputs():
    from sketchyscenecolorization_amd.trainer import Pix2PixTrainer
    z, p, b = _load()
    tr = Pix2PixTrainer(img=64, seed=3)
    tr.store.load_dict(p)
    dev = {k: (v.cuda() if k != 'text' else v.numpy()) for k, v in b.items()}
    out = tr.generate(dev['sketches'], dev['text'], dev['noise_vec'])
    assert float((out.cpu() - torch.from_numpy(z['gen'])).abs().max()) < 1e-3
    ld = float(tr.d_gradients(dev))
    assert abs(ld - float(z['loss_d'])) < 1e-4
    for k in z.files:
        if k.startswith('l2_discriminator'):
            name = k[3:].replace('.', '/')
            assert abs(float(tr.store.discriminator.g[name].norm()) - float(z[k])) < 5e-3 * float(z[k])
    lg = float(tr.g_gradients(dev))
    assert abs(lg - float(z['loss_g'])) < 1e-4
    for k in z.files:
        if k.startswith('l2_generator'):
            name = k[3:].replace('.', '/')
            assert abs(float(tr.store.generator.g[name].norm()) - float(z[k])) < 5e-3 * float(z[k])


# --------------------------------------------------------------------------- Residual / MRU / BG variants
def _variants():
    import importlib.util
    spec = importlib.util.spec_from_file_location('make_variant_goldens', os.path.join(GOLD, 'make_variant_goldens.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m, np.load(os.path.join(GOLD, 'variants_seed0_42.npz'))


def test_variant_oracles_reproduce_frozen_outputs():
    from oracle import mru as M
    from oracle import residual as R
    m, z = _variants()
    b = m.inputs(64)
    p = R.init_params('fg', seed=0, with_discriminator=True, img=64)
    # fp32 reduction order follows the host's thread count and instruction set: the float64 graph is pinned, the fp32 image is held
    # to the frozen one within 5e-5 or within 1.5 x its own distance from float64 (as the BG clause below)
    gen = R.generate_residual(p, b['sketches'], b['text'], b['noise_vec'])
    gen64 = R.generate_residual(m.to_f64(p), b['sketches'].double(), b['text'], b['noise_vec'].double())
    assert np.abs(gen64.numpy() - z['residual_gen_f64']).max() < 1e-9
    own = float((gen.double() - gen64).abs().max())
    assert own < 1e-3 and float(np.abs(z['residual_gen'] - gen64.numpy()).max()) < 1e-3
    assert float(np.abs(gen.numpy() - z['residual_gen']).max()) < max(5e-5, 1.5 * own)
    disc, logit = R.discriminate_residual(p, b['sketches'], b['images_d'])
    assert np.abs(logit.numpy() - z['residual_real_logit']).max() < 5e-5
    pm = M.init_params(0, img=64)
    gm = M.generate_mru(pm, b['sketches'], b['text'], b['class_id'], b['noise_vec']).numpy()
    assert np.abs(gm - z['mru_gen']).max() < 5e-5
    pb = R.init_params('bg', seed=0, img=96)
    x, text = m.bg_inputs()
    img, seg = R.create_residual_generator(pb, x, text)
    # The 96x96 batch-norm stack amplifies fp32 rounding: the fp32 oracle sits up to 2e-3 from its own float64 evaluation, and
    # by how much depends on the host's conv kernels (an AVX-512 box reads 9e-4 against the frozen fp32 image of the box that
    # froze it).  The float64 graph is the host-independent pin; the fp32 one is held to its own distance from float64.
    img64, seg64 = R.create_residual_generator(m.to_f64(pb), x.double(), text)
    assert np.abs(img64.numpy() - z['bg_image_f64']).max() < 1e-9
    assert np.abs(seg64.numpy() - z['bg_region_logits_f64']).max() < 1e-9
    for got, ref64, frozen in ((img, img64, z['bg_image']), (seg, seg64, z['bg_region_logits'])):
        own = float(np.abs(got.double().numpy() - ref64.numpy()).max())
        assert own < 5e-3
        assert float(np.abs(frozen - ref64.numpy()).max()) < 5e-3
        assert float(np.abs(got.numpy() - frozen).max()) < max(2e-4, 1.5 * own)


@pytest.mark.gpu
def test_hip_variants_match_frozen_outputs():
    from oracle import mru as M
    from oracle import residual as R
    from sketchyscenecolorization_amd import bg_colorization as bg
    from sketchyscenecolorization_amd.mru import MRUGenerator
    from sketchyscenecolorization_amd.params import Buffers, ParamStore
    from sketchyscenecolorization_amd.trainer import GanTrainer
    m, z = _variants()
    b = m.inputs(64)
    dev = {k: (v.cuda() if k != 'text' else v.numpy()) for k, v in b.items()}
    tr = GanTrainer(img=64, seed=3, block_type='Residual')
    tr.store.load_dict(R.init_params('fg', seed=0, with_discriminator=True, img=64))
    out = tr.generate(dev['sketches'], dev['text'], dev['noise_vec'])
    assert float((out.cpu() - torch.from_numpy(z['residual_gen'])).abs().max()) < 1e-3
    assert abs(float(tr.d_gradients(dev)) - float(z['residual_loss_d'])) < 1e-3
    assert abs(float(tr.g_gradients(dev)) - float(z['residual_loss_g'])) < 1e-3 * float(z['residual_loss_g'])
    store = ParamStore('MRU', 58, 64, 'cuda', 0)
    store.load_dict(M.init_params(0, img=64))
    g = MRUGenerator(store, Buffers('cuda'))
    ctx = g.forward(dev['sketches'], dev['text'], dev['class_id'], dev['noise_vec'])
    assert float((g.output_nchw(ctx).cpu() - torch.from_numpy(z['mru_gen'])).abs().max()) < 1e-3
    bg.reset()
    bg.get_tower(96)[0].load_dict(R.init_params('bg', seed=0, img=96))
    x, text = m.bg_inputs()
    img, seg = bg.create_residual_generator(x, 3, text)
    assert float((img.cpu() - torch.from_numpy(z['bg_image'])).abs().max()) < 3e-3
    assert float((seg.cpu() - torch.from_numpy(z['bg_region_logits'])).abs().max()) < 3e-3
