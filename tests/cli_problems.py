"""Small in-memory problems for the command-line tests (train.main(argv, problem=...))."""
import numpy as np
from scipy import sparse

from conftest import pkg


def sparse_problem(task, cuda=True):
    """A 900-node sparse problem (the builder of the probe and link-eval CLI tests): features normal, targets one bit
    per class from the features' signs (multilabel, C = 4), their arg-max over five columns (classification), or a
    column (regression); folds 600 / 150 / 150, row 0 the dummy."""
    gs = pkg()
    rng = np.random.RandomState(0)
    n, D = 900, 12
    degs = rng.randint(1, 12, size=n + 1)
    degs[0] = 0
    rows = np.repeat(np.arange(n + 1), degs)
    cols = np.concatenate([np.arange(d) for d in degs])
    adj = sparse.csr_matrix((rng.randint(1, n + 1, size=rows.shape[0]), (rows, cols)))
    feats = rng.normal(size=(n + 1, D)).astype(np.float32)
    feats[0] = 0
    folds = np.array(["train"] * 601 + ["val"] * 150 + ["test"] * 150)
    folds[0] = "dummy"
    if task == "multilabel_classification":
        C, targets = 4, (feats[:, :4] > 0).astype(np.float32)
    elif task == "classification":
        C, targets = 5, np.argmax(feats[:, :5], axis=1).astype(np.int64).reshape(-1, 1)
    else:
        C, targets = 1, feats[:, :1].copy()
    return gs.NodeProblem.from_arrays(task, C, adj, adj, feats, folds, targets, cuda=cuda)
