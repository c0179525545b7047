"""VICReg variance-covariance loss, host side: the float64 restatement (tests/vicreg_cases.py) against the fixtures the REFERENCE's
function wrote (tests/golden/make_vicreg_golden.py), and the public surface -- signature, edge cases, config key, model argument."""
import inspect
import os

import numpy as np
import pytest
import torch

from vicreg_cases import vicreg_f64

CASES = ["a", "b", "c", "d", "e"]


def _fx(golden_dir, case):
    return np.load(os.path.join(golden_dir, f"vicreg_{case}.npz"))


def _kw(fx):
    return dict(variance_weight=float(fx["variance_weight"]), covariance_weight=float(fx["covariance_weight"]),
                variance_target=float(fx["variance_target"]), eps=float(fx["eps"]))


@pytest.mark.parametrize("case", CASES)
def test_restatement_matches_reference_fixture(golden_dir, case):
    fx = _fx(golden_dir, case)
    losses, grad = vicreg_f64(torch.from_numpy(fx["x"]), **_kw(fx))
    for got, want in zip(losses, fx["loss64"]):
        assert abs(got - want) <= 1e-12 * max(1.0, abs(want))
    assert np.abs(grad.numpy() - fx["grad64"]).max() <= 1e-12 * max(np.abs(fx["grad64"]).max(), 1e-30)
    assert os.path.getsize(os.path.join(golden_dir, f"vicreg_{case}.npz")) < 256 * 1024


def test_fixture_cases_are_the_ones_they_claim(golden_dir):
    shapes = {c: _fx(golden_dir, c)["x"].shape for c in CASES}
    assert shapes == {"a": (300, 64), "b": (400, 12), "c": (150, 128), "d": (257, 64), "e": (2, 20)}
    b = _fx(golden_dir, "b")
    std = torch.from_numpy(b["x"]).double().std(dim=0)
    assert (std < 1.0).any() and (std > 1.0).any()                       # hinge active on part of the columns only
    d = _fx(golden_dir, "d")["x"]
    assert abs(d.mean() - 50.0) < 0.1 and abs(d.std(axis=0).mean() - 0.5) < 0.05   # |mu| = 100 std: the cancellation case
    e = _fx(golden_dir, "e")
    assert np.ptp(e["x"][:, 3]) == 0.0 and float(e["variance_weight"]) == 0.0


def test_signature_matches_reference():
    from frl_hip.losses import covariance_loss, variance_covariance_loss, variance_loss
    sig = inspect.signature(variance_covariance_loss)
    assert list(sig.parameters) == ["embeddings", "variance_weight", "covariance_weight", "variance_target", "eps"]
    assert [p.default for p in list(sig.parameters.values())[1:]] == [1.0, 1.0, 1.0, 1e-4]
    sv = inspect.signature(variance_loss)
    assert list(sv.parameters) == ["embeddings", "target", "eps"] and [p.default for p in list(sv.parameters.values())[1:]] == [1.0, 1e-4]
    sc = inspect.signature(covariance_loss)
    assert list(sc.parameters) == ["embeddings", "eps"] and sc.parameters["eps"].default == 1e-4


def test_edge_cases_on_the_host():
    from frl_hip.losses import covariance_loss, variance_covariance_loss, variance_loss
    for fn in (variance_covariance_loss, variance_loss, covariance_loss):
        with pytest.raises(ValueError):
            fn(torch.zeros(2, 3, 4))
    out = variance_covariance_loss(torch.randn(1, 8))                    # N < 2: three zeros, nothing is launched (CPU tensor accepted)
    assert len(out) == 3 and all(float(o) == 0.0 for o in out)
    assert float(variance_loss(torch.randn(1, 8))) == 0.0 and float(covariance_loss(torch.randn(1, 8))) == 0.0
    # float32 like every N >= 2 result, whatever the row dtype
    assert all(o.dtype == torch.float32 for o in variance_covariance_loss(torch.randn(1, 8).to(torch.bfloat16)))
    from frl_hip._lib import FrlHipError
    with pytest.raises(FrlHipError, match="GPU"):                        # product path: no CPU fallback
        variance_covariance_loss(torch.randn(16, 8))


def test_ops_refuse_cpu_tensors():
    from frl_hip import ops
    with pytest.raises(Exception, match="GPU"):
        ops.vicreg_fwd(torch.randn(16, 8))
    with pytest.raises(Exception, match="GPU"):
        ops.vicreg_bwd(torch.randn(16, 8), torch.zeros(8, 8), torch.zeros(2, 8), torch.ones(3))


def test_config_and_model_accept_lambda_vcr(tmp_path):
    from frl_hip.config import VAEConfig, load_vae_config
    from frl_hip.models import VQVAE
    cfg = VAEConfig()
    assert cfg.lambda_vcr == 0.0 and cfg.vcr_variance_weight == 1.0 and cfg.vcr_covariance_weight == 1.0 and cfg.vcr_variance_target == 1.0
    p = tmp_path / "c.yaml"
    p.write_text("lambda_vcr: 0.1\nvcr_variance_weight: 25.0\n")
    cfg = load_vae_config(str(p))
    assert cfg.lambda_vcr == 0.1 and cfg.vcr_variance_weight == 25.0 and "lambda_vcr" not in cfg.extra
    kw = dict(in_features=8, codebook_size=16, emb_dim=8, hidden=16, z_phase_dim=4, type_encoder_channels=(16, 8), type_encoder_num_groups=4,
              spatial_conv_gate_hidden=8, phase_tcn_channels=(8, 8, 8), phase_tcn_num_groups=4)
    m = VQVAE(lambda_vcr=0.5, vcr_variance_weight=25.0, vcr_covariance_weight=2.0, vcr_variance_target=0.5, **kw)
    assert (m.lambda_vcr, m.vcr_variance_weight, m.vcr_covariance_weight, m.vcr_variance_target) == (0.5, 25.0, 2.0, 0.5)
    assert VQVAE(**kw).lambda_vcr == 0.0
    assert "lambda_vcr" in inspect.signature(VQVAE.__init__).parameters
    with pytest.raises(ValueError):
        VQVAE(lambda_vcr=-1.0, **kw)


def test_config_passes_the_term_to_the_model():
    from frl_hip.config import VAEConfig, _vcr_kwargs
    assert _vcr_kwargs(VAEConfig()) == {}                                # absent / zero: the model is built as before
    cfg = VAEConfig(lambda_vcr=0.1, vcr_variance_weight=25.0)
    assert _vcr_kwargs(cfg) == dict(lambda_vcr=0.1, vcr_variance_weight=25.0, vcr_covariance_weight=1.0, vcr_variance_target=1.0)
