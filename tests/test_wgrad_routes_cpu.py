"""The weight-gradient route table (tests/wgrad_routes.py) is whole -- every row has its recorded facts, every row of tests/grad_routes.py
is in it -- and the library's workspace functions (host code) give each row's recorded size; the image-row rows split as the table's
docstring says.  Runs without a GPU."""
import grad_routes as G
import wgrad_routes as R


def test_every_row_has_facts():
    assert [r["id"] for r in R.ROWS] == list(R.FACTS) and len(set(R.FACTS)) == len(R.ROWS)
    assert {"g." + r["id"] for r in G.ROWS} <= set(R.FACTS)
    for launches, wsb, sha in R.FACTS.values():
        assert len(sha) == 64 and set(sha) <= set("0123456789abcdef"), sha
        assert launches == 2 and wsb > 0   # the kernel and its ordered reduce; slabs come out of the workspace


def test_workspace_bytes_of_every_row():
    got = {r["id"]: R.workspace_bytes(r) for r in R.ROWS}
    assert got == {k: f[1] for k, f in R.FACTS.items()}


def test_image_row_split_counts():
    """S = workspace / (N x Kpad floats), K = 288 -> Kpad = 384: 24 (quarter sums), 10 and 5 (one sum per element)."""
    for tag, _B, _H, S in R.ROW_SIZES:
        rows = [r for r in R.ROWS if r["id"].startswith("row.%s." % tag)]
        assert len(rows) == 9
        for r in rows:
            assert R.workspace_bytes(r) == S * r["N"] * 384 * 4, r["id"]
