"""ssc_match_score (csrc/match_val.hip) restated in NumPy, in float64 and in float32, for tests/test_match_validation.py and
tests/test_gpu_match_validation.py: the legacy bilinear up-sampling of pred (tests/matching_oracle.py::resize_bilinear_legacy, the
order of operations of the kernel), then per pixel b = sketch[..., 0], z = lut[labels] != 0 and

    I = #{u >= 1e-9 && b != 255 && z}   P = #{u >= 1e-9 && b != 255}   A = #{z}   live = #{b <= 104}
    loss = sum over the live pixels of max(u, 0) - u z + log1p(exp(-|u|))

The threshold is the float32 number 1e-9f in both precisions, as on the device.  -> {I, P, A, live, loss, U, up, predicts}."""
import numpy as np

import matching_oracle as MO

THRESHOLD = np.float32(1e-9)


def score(pred, sketch, labels, lut, dtype=np.float64):
    dt = np.dtype(dtype)
    pred = np.asarray(pred, dtype=np.float32)
    sketch, labels, lut = (np.asarray(a, dtype=np.uint8) for a in (sketch, labels, lut))
    S = labels.shape[0]
    assert labels.shape == (S, S) and sketch.shape == (S, S, 3) and lut.shape == (256,)
    up = MO.resize_bilinear_legacy(pred.astype(dt), S, dt)
    assert up.dtype == dt
    b = sketch[:, :, 0]
    z = lut[labels] != 0
    on = (up >= dt.type(THRESHOLD)) & (b != 255)
    live = b <= 104
    u = up[live]
    terms = np.maximum(u, dt.type(0)) - u * z[live].astype(dt) + np.log1p(np.exp(-np.abs(u)))
    assert terms.dtype == dt
    I, P, A = int((on & z).sum()), int(on.sum()), int(z.sum())
    return {'I': I, 'P': P, 'A': A, 'live': int(live.sum()), 'loss': float(terms.astype(np.float64).sum()),
            'abs_terms': float(np.abs(terms.astype(np.float64)).sum()), 'U': P + A - I, 'up': up, 'predicts': on.astype(np.uint8)}
