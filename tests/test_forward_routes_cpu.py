"""The forward route table (tests/forward_routes.py) is whole -- every row has its recorded facts, every route the dispatch has is in it --
and the library's workspace function (host code) gives each row's recorded size.  Runs without a GPU."""
import forward_routes as R


def test_every_row_has_facts_and_every_route_a_row():
    assert [r["id"] for r in R.ROWS] == list(R.FACTS) and len(set(R.FACTS)) == len(R.ROWS)
    labels = [f[0] for f in R.FACTS.values()]
    missing = [want for want in R.REQUIRED_LABELS if want not in labels]
    assert not missing, missing
    reduced = {lab for lab in labels if lab.startswith("igemm_f32<") and lab.endswith(" + split-K reduce")}
    assert len(reduced) >= 2, reduced
    for label, launches, wsb, sha in R.FACTS.values():
        assert len(sha) == 64 and set(sha) <= set("0123456789abcdef"), sha
        assert launches == (2 if label.endswith(" + split-K reduce") else 1) and wsb >= 0
        assert wsb > 0 or not label.endswith(" + split-K reduce")   # slabs come out of the workspace


def test_workspace_bytes_of_every_row():
    got = {r["id"]: R.workspace_bytes(r) for r in R.ROWS}
    assert got == {k: f[2] for k, f in R.FACTS.items()}
