"""forward_tiles with x_type taken from the phase encoder's forward launch (VQVAE.chain_xtype) against the separate mean_time pass:
x_type is the same tensor bit for bit, so every output, gradient and parameter trajectory must be too -- eager and graph-captured,
with the phase branch on its own stream and on the main stream."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _model(chain_xtype=True, concurrent=True):
    from frl_hip.models import VQVAE
    torch.manual_seed(0)
    m = VQVAE(in_features=64, codebook_size=32, emb_dim=64, beta=0.25, type_encoder_dropout=0.0, phase_tcn_dropout=0.0,
              compute_dtype=torch.bfloat16).to(DEV)
    with torch.no_grad():
        m.quant.codebook.copy_(torch.randn(32, 64, generator=_gen(7)))
    m.chain_xtype = chain_xtype
    m.concurrent_phase = concurrent
    return m


def _tiles(n):
    g = _gen(13)
    return [torch.randn(2, 5, 8, 8, 64, generator=g).to(torch.bfloat16).to(DEV) for _ in range(n)]


@pytest.fixture(scope="module")
def reference_step():
    """One forward_tiles + backward with the separate mean_time pass, two streams: (outputs, gradients).  Left unchanged by its users."""
    return _one_step(_model(chain_xtype=False), _tiles(1)[0])


def _one_step(m, tile):
    out = m.forward_tiles(tile)
    out["loss"].backward()
    torch.cuda.synchronize()
    outs = {k: v.detach().clone() for k, v in out.items() if torch.is_tensor(v)}
    return outs, {n: p.grad.clone() for n, p in m.named_parameters()}


def _same(a, b):
    if a.dtype == torch.bfloat16:
        return torch.equal(a.view(torch.int16), b.view(torch.int16))
    return torch.equal(a, b)


@pytest.mark.parametrize("concurrent", [True, False])
def test_step_with_x_type_from_the_chain_equals_the_mean_time_step(reference_step, concurrent, monkeypatch):
    from frl_hip import ops
    calls = []
    real = ops.mean_time
    monkeypatch.setattr(ops, "mean_time", lambda t: (calls.append(1), real(t))[1])
    outs, grads = _one_step(_model(True, concurrent), _tiles(1)[0])
    assert not calls, "the mean_time pass still ran"
    ref_outs, ref_grads = reference_step
    assert set(outs) == set(ref_outs) and set(grads) == set(ref_grads)
    for k in ref_outs:
        assert _same(outs[k], ref_outs[k]), k
    for n in ref_grads:
        assert torch.equal(grads[n], ref_grads[n]), n
    # the switch: off means the separate pass
    _one_step(_model(False, concurrent), _tiles(1)[0])
    assert len(calls) == 1


def test_configurations_outside_the_hot_chain_keep_mean_time(monkeypatch):
    """float32 compute (no one-launch chain) and the legacy contract still take x_type from ops.mean_time."""
    from frl_hip import ops
    from frl_hip.models import VQVAE
    calls = []
    real = ops.mean_time
    monkeypatch.setattr(ops, "mean_time", lambda t: (calls.append(1), real(t))[1])
    m = VQVAE(in_features=8, codebook_size=16, emb_dim=8, beta=0.25, hidden=16, z_phase_dim=4, type_encoder_channels=(16, 8),
              type_encoder_dropout=0.0, type_encoder_num_groups=4, spatial_conv_gate_hidden=8, phase_tcn_channels=(8, 8, 8),
              phase_tcn_dropout=0.0, phase_tcn_num_groups=4).to(DEV)
    m.forward_tiles(torch.randn(2, 5, 8, 8, 8, generator=_gen(3)).to(DEV))
    assert len(calls) == 1
    _model().forward_tiles(_tiles(1)[0], differentiable_vq_loss=True)
    assert len(calls) == 2


def test_graph_captured_steps_equal_eager_steps_with_x_type_from_the_chain():
    """The new dependency (type path waits for the chain on the phase stream) is captured like the existing fork and join: three
    step_graphed steps end in the parameters of three eager steps, and those in the parameters of the mean_time trainer."""
    from frl_hip.training.trainer import VQVAETrainer
    tiles = _tiles(3)
    runs = {}
    for name, (xt, graphed) in {"eager": (True, False), "graphed": (True, True), "mean_time": (False, False)}.items():
        m = _model(chain_xtype=xt)
        tr = VQVAETrainer(m, lr=1e-3, total_steps=10)
        losses = [float((tr.step_graphed(t) if graphed else tr.step(t))["loss"].detach()) for t in tiles]
        torch.cuda.synchronize()
        if graphed:
            assert tr.graph_supported()
        runs[name] = (m, losses)
    for other in ("graphed", "mean_time"):
        assert runs["eager"][1] == runs[other][1], other
        for (n, p), (_, p1) in zip(runs["eager"][0].named_parameters(), runs[other][0].named_parameters()):
            assert torch.equal(p, p1), (other, n)
