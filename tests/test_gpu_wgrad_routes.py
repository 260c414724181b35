"""GPU: every row of tests/wgrad_routes.py through its weight-gradient entry with the row's knobs and arithmetic and the workspace the
library's own function asks for -- the launches the call made (m2h_launch_count), the workspace size and the SHA-256 of the gradient's
bytes are the ones recorded in the table.  The table holds observations, not a restatement of the dispatch: see its docstring."""
import hashlib

import pytest
import torch

import wgrad_routes as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("row", R.ROWS, ids=[r["id"] for r in R.ROWS])
def test_wgrad_route(row):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    dw, launches, wsb = R.run(row, torch.device("cuda", 0))
    sha = hashlib.sha256(dw.cpu().numpy().tobytes()).hexdigest()
    print("%s: %d launch(es), %d workspace bytes, sha256 %s" % (row["id"], launches, wsb, sha))
    assert (launches, wsb, sha) == R.FACTS[row["id"]]
    assert bool(torch.isfinite(dw).all()) and float(dw.abs().max()) > 0   # the launches wrote the gradient
