"""Helper run as a subprocess by tests/test_gpu_checkpoint.py (not a test module): a fresh process loads a
checkpoint file, runs the chain to its end and writes everything test_gpu_checkpoint._collect gathers.

usage: gpu_checkpoint_run.py <checkpoint.npz> <result.npz> <n_samples>"""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, HERE]
PKG = "laurabaracaldo-spatial-meta-kriging-for-distributed-inference-for-binary-response_amd"


def main():
    path, res, n = sys.argv[1], sys.argv[2], int(sys.argv[3])
    mk = importlib.import_module(PKG)
    from test_gpu_checkpoint import _collect
    with mk.fitfile.load_checkpoint(path) as ses:
        assert ses.kernel_stats(mk.session.KS_ITER)["launches"] == 0
        ses.run(n - ses.iteration)
        got = _collect(ses)
    np.savez(res, **got)


if __name__ == "__main__":
    main()
