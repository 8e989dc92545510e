"""CPU: the inputs of test_featscreen_bias_gpu.py / test_featscreen_bounds_gpu.py
are adversarial by construction, checked in numpy with no rule for the bias B
assumed (featscreen_cases.py restates the packs' scale and row_tail's bound)."""
import numpy as np
import pytest

import featscreen_cases as fc


@pytest.mark.parametrize("name", list(fc.BIAS_CASES))
def test_boundary_case_is_adversarial(name):
    """Each boundary row's twin value falls below B - |x s|^2 by more than the
    distance from |x s|^2 to the next power of two, its runner-up gap is above
    4 bnd in both directions, and the pair is flagged for the repair pack exactly
    in the `tail` variants."""
    fc.check_boundary_pair(fc.BIAS_CASES[name])


def test_boundary_batch_is_adversarial():
    ps, F, G = fc.bias_batch()
    assert F.shape == (5, 520, 32) and G.shape == (5, 480, 32)
    scales = []
    for p in (0, 2, 4):
        fc.check_boundary_pair(ps[p])
        scales.append(fc.pair_scale(F[p], G[p])[0])
    assert len(set(scales)) == 3  # three magnitudes: three scales, three biases


@pytest.mark.parametrize("name", list(fc.ONESIDED_CASES))
def test_onesided_case_is_adversarial(name):
    fc.check_onesided_pair(fc.ONESIDED_CASES[name])


def test_model_boundary_twin_value():
    """The model on the smallest instance: D = 32, a = 1 - 2^-13, scale 2^11:
    |x s|^2 = 2^27 (1 - 2^-13)^2, f16(a s) = 2^11, and with the smallest power of
    two above |x s|^2 as the bias the twin's value f32(|y s|^2 + B) - 2 |f16(x s)|^2
    is -32768."""
    x = np.full((1, 32), 1.0 - 2.0 ** -13, np.float32)
    s = fc.pair_scale5(x.max(), 11)
    assert s == 2.0 ** 11
    n2, h2, _, _ = fc.scaled_terms(x, s)
    assert h2[0] == 2.0 ** 27 and n2[0] < 2.0 ** 27
    ct = np.float32(np.float32(n2[0]) + np.float32(2.0 ** 27))
    assert float(ct) - 2.0 * h2[0] == -32768.0


def test_synthetic_4096_bound_can_decide():
    """The certificate is not vacuous on ordinary data: for more than half of
    synthetic_4096's rows the modelled per-value bound 0.5 bnd + ebias (at a bias
    no rule exceeds) is below half the row's exact top-2 gap."""
    from pointcloudregistration_amd import synth
    B = synth.make_batch(1, n=4096, m=4096, d=32, base_seed=77, feat_noise=1.0)
    F, G = np.asarray(B.src_feat[0], np.float32), np.asarray(B.tgt_feat[0], np.float32)
    s, _ = fc.pair_scale(F, G)
    _, _, exf, qf = fc.scaled_terms(F, s)
    _, _, exg, qg = fc.scaled_terms(G, s)
    d = np.partition(fc.exact_dist(F, G), 1, axis=1)[:, :2] * s * s
    bnd, ebias = fc.bnd_ct(qf, exf, qg.max(), exg.max(), fc.bias_upper(max(qf.max(), qg.max())), 32)
    e = (0.5 * bnd + ebias) * (1.0 + 1e-6)
    assert (e < 0.5 * (d[:, 1] - d[:, 0])).mean() > 0.5
