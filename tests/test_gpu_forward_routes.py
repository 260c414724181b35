"""GPU: every row of tests/forward_routes.py through m2h_conv_igemm_f32 with default knobs and the workspace the library's own
function asks for -- the kernel that ran (m2h_last_kernel), the launches the call made (m2h_launch_count), the workspace size and the
SHA-256 of the output's bytes are the ones recorded in the table.  The table holds observations, not a restatement of the dispatch: see its docstring."""
import hashlib

import pytest
import torch

import forward_routes as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("row", R.ROWS, ids=[r["id"] for r in R.ROWS])
def test_forward_route(row):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    out, label, launches, wsb = R.run(row, torch.device("cuda", 0))
    torch.cuda.synchronize()
    sha = hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()
    print("%s: %s, %d launch(es), %d workspace bytes, sha256 %s" % (row["id"], label, launches, wsb, sha))
    assert (label, launches, wsb, sha) == R.FACTS[row["id"]]
    assert bool(torch.isfinite(out).all()) and float(out.abs().max()) > 0   # the launch wrote the output
