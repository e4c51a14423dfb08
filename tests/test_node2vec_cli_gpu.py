"""End-to-end: train_student.py with every node2vec switch of the position features on (biased walks, degree^0.75 negatives, a context
table; docs/POSITION_SEMANTICS.md) distils an MLP student whose input is [features | position embedding], transductive and inductive.  The
output directory leaf is the one --position_dim alone gives."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(script, args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, script)] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


@pytest.mark.parametrize("setting", ["tran", "ind"])
def test_student_cli_with_node2vec_position_features(tmp_path, setting):
    common = ["--dataset", "synthetic-cora", "--teacher", "GCN", "--device", "0", "--max_epoch", "3", "--patience", "3",
              "--exp_setting", setting, "--save_results"]
    _run("train_teacher.py", common, tmp_path)
    base = tmp_path / "outputs" / ("transductive" if setting == "tran" else "inductive/split_rate_0.2") / "synthetic-cora"
    _run("train_student.py", common + ["--student", "MLP", "--position_dim", "16", "--position_epochs", "2", "--position_p", "0.5",
                                       "--position_q", "2", "--position_negative_power", "0.75", "--position_context_table"], tmp_path)
    sdir = base / "GCN_PE16MLP" / "seed_0"
    out_s = np.load(sdir / "out.npz")["arr_0"]
    assert out_s.shape == (2485, 7) and np.isfinite(out_s).all()
    np.testing.assert_allclose(np.exp(out_s).sum(1), 1.0, atol=1e-4)
    sd = torch.load(sdir / "model.pth", map_location="cpu")
    first = [v for k, v in sd.items() if k.endswith("layers.0.weight")]
    assert len(first) == 1 and first[0].shape[1] == 1433 + 16
    log = (sdir / "log").read_text()
    assert "position embedding" in log
    losses = [float(x) for x in log.split("loss per epoch")[1].split("\n")[0].split()]
    assert len(losses) == 2 and all(np.isfinite(losses))
