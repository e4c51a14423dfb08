"""End-to-end: a train_student.py --position_dim 16 --save_results run leaves position.npz beside model.pth, and serve_student.py serves
the run by node id from those artefacts (docs/POSITION_SEMANTICS.md, "Serving by node id"), transductive and inductive.  The served
log-probabilities are held to the run's own out.npz within 1e-4 absolute, the project's fp32 parity bar: out.npz is the same best-state
model over cat([X, dense]), and the rows of unseen nodes differ by summation order only."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(script, args, cwd, ok=True):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, script)] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert (r.returncode == 0) == ok, r.stderr[-3000:]
    return r


@pytest.mark.parametrize("setting", ["tran", "ind"])
def test_serve_student_cli(tmp_path, setting):
    common = ["--dataset", "synthetic-cora", "--teacher", "GCN", "--device", "0", "--exp_setting", setting]
    train = common + ["--max_epoch", "3", "--patience", "3", "--save_results"]
    _run("train_teacher.py", train, tmp_path)
    base = tmp_path / "outputs" / ("transductive" if setting == "tran" else "inductive/split_rate_0.2") / "synthetic-cora"
    _run("train_student.py", train + ["--student", "MLP", "--position_dim", "16", "--position_epochs", "2"], tmp_path)
    sdir = base / "GCN_PE16MLP" / "seed_0"
    with np.load(sdir / "position.npz") as t:
        rows, node_ids, num_nodes = t["rows"], t["node_ids"], int(t["num_nodes"])
    assert rows.dtype == np.float32 and rows.shape[1] == 16 and num_nodes == 2485 and node_ids.shape == (rows.shape[0],)
    if setting == "tran":
        assert rows.shape[0] == 2485 and np.array_equal(node_ids, np.arange(2485))
    else:
        from glnn_amd.dataloader import load_data
        from glnn_amd.utils import graph_split
        _, _, idx_train, idx_val, idx_test = load_data("synthetic-cora", "./data", split_idx=0, seed=0, labelrate_train=20, labelrate_val=30)
        idx_obs = graph_split(idx_train, idx_val, idx_test, 0.2, 0)[3]
        assert 0 < rows.shape[0] < 2485 and np.array_equal(node_ids, np.asarray(idx_obs))
    serve = common + ["--student", "MLP", "--position_dim", "16", "--serve_dtype", "float32"]
    _run("serve_student.py", serve, tmp_path)
    served = np.load(sdir / "served_out.npz")["arr_0"]
    out = np.load(sdir / "out.npz")["arr_0"]
    assert served.shape == (2485, 7) and served.dtype == np.float32
    print(f"{setting}: max |served - out.npz| = {np.abs(served - out).max():.3e}")
    assert np.abs(served - out).max() <= 1e-4
    # a second run over ten ids: the corresponding rows of the first, bit for bit
    ids = np.array([2484, 0, 7, 7, 1200, 33, 2000, 1, 999, 512], np.int64)
    np.save(tmp_path / "ids.npy", ids)
    _run("serve_student.py", serve + ["--nodes", str(tmp_path / "ids.npy")], tmp_path)
    ten = np.load(sdir / "served_out.npz")["arr_0"]
    assert ten.shape == (10, 7) and np.array_equal(ten.view(np.int32), served[ids].view(np.int32))
    # the plain run writes no position.npz, and serve_student.py refuses it by name
    _run("train_student.py", train + ["--student", "MLP"], tmp_path)
    assert (base / "GCN_MLP" / "seed_0" / "model.pth").exists() and not (base / "GCN_MLP" / "seed_0" / "position.npz").exists()
    r = _run("serve_student.py", common + ["--student", "MLP"], tmp_path, ok=False)
    assert "no position.npz" in r.stderr
