#!/usr/bin/env python
"""`python serve_student.py --teacher SAGE --student MLP --dataset ... --position_dim D --device 0 [--nodes ids.npy]`: log-probabilities
of a position-feature student by node id, from the artefacts of a finished `train_student.py --position_dim D --save_results` run
(model.pth, position.npz); see glnn_amd/cli.py and docs/POSITION_SEMANTICS.md."""
from glnn_amd.cli import serve_main

if __name__ == "__main__":
    serve_main()
