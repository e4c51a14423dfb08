"""The one table of model families (glnn_amd.kinds) and what reads it: the order rule of the keys, the name's resolution, the step every
full-graph family has, the sharding refusals, the paths the rows name, the three generated name lists, and the construction order of
the two stack encoders that share models._ConvStack.  No GPU call is made."""
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "graphless-neural-networks_amd")


def _rows():
    from glnn_amd.kinds import KINDS
    return KINDS


def _full_graph_keys():
    return [row.key for row in _rows() if row.full_graph]


def test_keys_and_kinds_are_unique_and_a_key_stands_in_front_of_every_key_it_contains():
    keys, kinds = [row.key for row in _rows()], [row.kind for row in _rows()]
    assert len(set(keys)) == len(keys) == len(set(kinds)) and keys[0] == "MLP"
    pairs = [(a, b) for a in keys for b in keys if a != b and b in a]
    assert ("GCNII", "GCN") in pairs and ("GATv2", "GAT") in pairs
    for longer, shorter in pairs:
        assert keys.index(longer) < keys.index(shorter), (longer, shorter)


def test_teacher_kind_maps_every_key_with_and_without_the_augmentation_prefix():
    from glnn_amd import kinds, models
    assert models.teacher_kind is kinds.teacher_kind and models.FULL_GRAPH_KINDS is kinds.FULL_GRAPH_KINDS
    for row in _rows():
        assert kinds.teacher_kind(row.key) == row.kind and kinds.teacher_kind("GA2" + row.key) == row.kind
        assert row.key in kinds.teacher_kind.__doc__ and kinds.BY_KIND[row.kind] is row and kinds.BY_KEY[row.key] is row
    assert "contains" in kinds.teacher_kind.__doc__
    assert kinds.FULL_GRAPH_KINDS == tuple(row.kind for row in _rows() if row.full_graph)
    assert {row.kind for row in _rows() if not row.full_graph} == {"mlp", "sage"}


def test_every_full_graph_kind_has_its_engine_step():
    from glnn_amd.teacher import TeacherEngine
    from glnn_amd.train_and_eval import _full_graph_step
    eng = TeacherEngine.__new__(TeacherEngine)
    for row in _rows():
        if row.full_graph:
            assert _full_graph_step(eng, row.key) == getattr(eng, "step_" + row.kind)
            assert row.rule in ("norm_relu", "attn", "stack", "gcn") and row.supported.startswith(row.key + " with ")
        else:
            with pytest.raises(NotImplementedError, match="no full-graph step"):
                _full_graph_step(eng, row.key)


@pytest.mark.parametrize("teacher", ["ShardedTeacher", "HaloShardedTeacher"])
def test_every_graph_kind_but_the_sharded_three_is_refused_with_its_reason(teacher):
    import glnn_amd.dist as gdist
    for row in _rows():
        if row.kind in ("mlp", "sage", "gcn", "appnp"):
            assert row.unsharded is None
            continue
        assert row.unsharded
        with pytest.raises(NotImplementedError) as e:
            getattr(gdist, teacher)(type(row.key, (), {})(), None, None, None)
        assert str(e.value) == (f"{teacher}: the {row.key} teacher is not sharded -- {row.unsharded}, an exchange the sharded forward does "
                                f"not have (whole-graph {row.key} only)")


def test_every_path_a_row_names_exists():
    for row in _rows():
        texts = [t for t in (row.supported, row.unsharded) + (row.bf16 or ()) if t]
        for path in re.findall(r"docs/\w+\.md", " ".join(texts)):
            assert os.path.exists(os.path.join(ROOT, path)), (row.key, path)
        if row.bf16:
            src, doc, section = row.bf16
            assert os.path.exists(os.path.join(PKG, src)) and os.path.exists(os.path.join(ROOT, doc)), row.key
            assert section in open(os.path.join(ROOT, doc)).read(), (row.key, section)
        assert all(name in [r.key for r in _rows()] for name in row.stand_ins)


def _exactly_once(msg, keys):
    words = re.findall(r"[A-Za-z0-9]+", msg)
    assert all(words.count(k) == 1 for k in keys), msg
    assert [w for w in words if w in keys] == keys, msg          # ... in the table's order


def test_the_generated_messages_name_every_full_graph_teacher_once(monkeypatch, capsys):
    from glnn_amd import teacher, train_and_eval
    from glnn_amd.cli import get_teacher_args
    stub = type("M", (), {"model_name": "SAGE", "encoder": None})()
    monkeypatch.setattr(teacher, "check_supported", lambda *a: None)
    with pytest.raises(NotImplementedError, match="the full-graph step is implemented for the") as e:
        train_and_eval.train(stub, None, None, None, None, None, None)
    _exactly_once(str(e.value).split("(SAGE trains")[0], _full_graph_keys())
    monkeypatch.undo()
    stub.model_name = "MLP"
    with pytest.raises(NotImplementedError, match="teachers only") as e:
        teacher.check_supported(stub, None, None)
    _exactly_once(str(e.value).split("(got")[0], ["SAGE"] + _full_graph_keys())
    with pytest.raises(SystemExit):
        get_teacher_args(["--teacher", "SAGE", "--subgraph_walk_length", "3"])
    err = capsys.readouterr().err
    _exactly_once(err[err.index("applies to the full-graph teachers"):].split(" only:")[0], _full_graph_keys())


def _stack_conf(name):
    return dict(model_name=name, num_layers=2, feat_dim=8, hidden_dim=16, label_dim=4, dropout_ratio=0.0, norm_type="none", device="cpu",
                pna_delta=1.25)


def _gcnii_weight():
    w = torch.empty(16, 16)
    torch.nn.init.uniform_(w, -1.0 / math.sqrt(16), 1.0 / math.sqrt(16))
    return {"weight": w}


def _linear(d_in, d_out):
    lin = torch.nn.Linear(d_in, d_out)
    return {"weight": lin.weight, "bias": lin.bias}


@pytest.mark.parametrize("name,layer", [("GCNII", lambda: {"": _gcnii_weight()}),
                                        ("PNA", lambda: {"pre.": _linear(32, 16), "post.": _linear(13 * 16, 16)})])
def test_stack_encoders_register_and_draw_in_the_order_written_out_by_hand(name, layer):
    """fc_in, the conv layers, fc_out (PNA: then the delta buffer): the state_dict keys in order, and the tensors torch's generator gives
    a hand-written sequence of the same constructions from the same seed."""
    from glnn_amd import models
    torch.manual_seed(7)
    m = models.Model(_stack_conf(name))
    assert isinstance(m.encoder, models._ConvStack) and type(m.encoder).__name__ == name
    torch.manual_seed(7)
    want = {"encoder.fc_in." + k: v for k, v in _linear(8, 16).items()}
    for l in range(2):
        want.update({f"encoder.layers.{l}.{sub}{k}": v for sub, part in layer().items() for k, v in part.items()})
    want.update({"encoder.fc_out." + k: v for k, v in _linear(16, 4).items()})
    assert [n for n, _ in m.named_parameters()] == list(want)
    sd = m.state_dict()
    assert list(sd) == (["encoder.delta"] if name == "PNA" else []) + list(want)       # (a module's own buffers come before its children)
    for k, v in want.items():
        assert torch.equal(sd[k], v), k
    assert list(m.encoder._modules) == ["dropout", "fc_in", "layers", "fc_out"]
