"""CPU checks of the two rules SAGE.inference's forms share: `_layer_tail` (what a layer's launch gets: the fused tail, or the conv's
bias alone when LayerNorm follows as a pass of its own) and `_chains_next` (whether layer l carries layer l+1's projection).  No call
into the library is made here."""
import pytest
import torch
import torch.nn.functional as F


def _sage(dims, norm="none", agg="gcn"):
    from glnn_amd.models import SAGE
    torch.manual_seed(0)
    return SAGE(len(dims) - 1, dims[0], dims[1], dims[-1], 0.5, F.relu, norm_type=norm, aggregator_type=agg).eval()


@pytest.mark.parametrize("agg", ["gcn", "mean"])
def test_layer_tail_without_norm_is_the_fused_tail(agg):
    m = _sage([20, 32, 32, 6], "none", agg)
    for l in range(3):
        scale, shift, relu, post_ln = m._layer_tail(l)
        assert (scale, shift, relu) == m._tail(l) and post_ln is False
        assert scale is None and relu is (l != 2)
        want = m.layers[l].fc_neigh.bias + (m.layers[l].fc_self.bias if agg == "mean" else 0)
        assert torch.equal(shift.detach(), want.detach())


@pytest.mark.parametrize("agg", ["gcn", "mean"])
def test_layer_tail_with_layernorm_keeps_the_hidden_tail_out_of_the_launch(agg):
    m = _sage([20, 32, 32, 6], "layer", agg)
    for l in range(2):                  # hidden: bias only, no ReLU, LayerNorm -> ReLU announced as a pass of its own
        scale, shift, relu, post_ln = m._layer_tail(l)
        assert scale is None and relu is False and post_ln is True
        if agg == "gcn":
            assert shift is m.layers[l].fc_neigh.bias
        else:
            assert torch.equal(shift, (m.layers[l].fc_self.bias + m.layers[l].fc_neigh.bias).detach())
        with pytest.raises(NotImplementedError, match="LayerNorm has per-row statistics"):
            m._tail(l)
    scale, shift, relu, post_ln = m._layer_tail(2)          # the last layer has no norm behind it
    assert (scale, shift, relu) == m._tail(2) and (scale, relu, post_ln) == (None, False, False)
    want = m.layers[2].fc_neigh.bias + (m.layers[2].fc_self.bias if agg == "mean" else 0)
    assert torch.equal(shift.detach(), want.detach())


@pytest.mark.parametrize("dims,want", [
    ([20, 32, 32, 6], [False, True, False]),        # layer 1 is fused and layer 2 (32 -> 6) projects first
    ([40, 24, 24, 6], [False, True, False]),        # layer 0 (40 -> 24) projects first itself: not fused, chains nothing
    ([20, 300, 300, 6], [False, False, False]),     # widths above 256: no layer is fused
])
def test_chains_next(dims, want, monkeypatch):
    from glnn_amd.models import SAGE
    m = _sage(dims)
    assert [m._chains_next(l) for l in range(3)] == want
    monkeypatch.setattr(SAGE, "CHAIN_NEXT_PROJECTION", False)
    assert [m._chains_next(l) for l in range(3)] == [False, False, False]


def test_chains_next_needs_a_narrowing_next_layer_of_at_most_256_columns():
    assert [_sage([20, 32, 32, 40])._chains_next(l) for l in range(3)] == [False, False, False]      # 32 -> 40 aggregates first
    assert [_sage([20, 32, 32])._chains_next(l) for l in range(2)] == [False, False]                 # 32 -> 32 too
    assert _sage([20, 32, 6])._chains_next(0) is True
