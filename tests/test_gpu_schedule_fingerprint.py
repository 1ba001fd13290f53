"""The launch schedule of the single-GPU drivers (csrc/potrf.hip, chain.hip, trsv.hip and their callers in api.hip, evidence.hip),
held to a recorded fingerprint: per profiling slot the number of launches and the flops, and the increments of every `route_*`
counter, for one run of every row below with profiling on for every slot.  Both are computed on the host from the launch shapes
(prof_begin, the route counters): they depend neither on the toolchain nor on timing, so a change of the host code that is meant
to leave every launch as it was must reproduce them -- launches and routes exactly, flops to a relative 1e-12 (the same sum in
the same order).

Rows: the first case of every route row of test_gpu_predict_backward.py (1 to 36 tile rows: fused and tile-by-tile solves,
look-ahead on and off, the two-level solve; the ride gated and ungated, in two halves, two-level, following the chain, back to
back, augmented); the factorisation alone on the T12 shape (one block) and the APP shape (three blocks factored, two appended in
one call) over the options that select its branches; the inverse diagonal, the single right-hand side and the backward solve.

The fixture is tests/golden/schedule_fingerprint.json.  A pull request that changes the schedule ON PURPOSE regenerates it on an
MI355X with
    python tests/test_gpu_schedule_fingerprint.py --write
and says so; any other difference is a launch that changed."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from _backward import Appender, restored  # noqa: E402
from test_gpu_predict_backward import APP, OPTIONS as PREDICT_OPTIONS, ROUTES, ROWS, T5, T12, Case, observation_points, routes  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(HERE, "golden", "schedule_fingerprint.json")
FLOPS_RTOL = 1e-12
OPTIONS = tuple(PREDICT_OPTIONS) + ("chain_resident_max_rows", "chain_resident2_max_rows", "chain_ahead", "nb_outer", "nb_outer_min_tiles",
                                    "append_split", "append_split_min_tiles", "inverse_diag_panel")

# (id, options): the factorisation alone, each on T12 (fresh) and on APP (blocks 0-2 factored, blocks 3-4 appended in one call)
FACTOR = [
    ("defaults", {}),
    ("lookahead0", {"lookahead": 0}),
    ("chain_resident_off", {"chain_resident_max_rows": -1}),
    ("chain_ahead0", {"chain_ahead": 0}),
    ("nb_outer1024", {"nb_outer": 1024, "nb_outer_min_tiles": 1}),
    ("append_split", {"append_split": 1, "append_split_min_tiles": 1}),
    ("chain_resident2_32", {"chain_resident2_max_rows": 32}),
    # (with the default chain_resident_max_rows = 32 no panel of these shapes is left to the two-launch form: this row reaches it)
    ("chain_resident2_32_after4", {"chain_resident_max_rows": 4, "chain_resident2_max_rows": 32}),
]
FACTOR_SHAPES = [("T12", T12, 0), ("APP", APP, 3)]


def _factored(ctx, blocks):
    X, noise = observation_points(sum(blocks))
    ap = Appender(ctx, X, noise)
    for nb in blocks:
        ap.add(nb)
        assert ap.mat.potrf() == 0
    return ap


def _run_predict(ctx, row):
    _, kind, _, cases, _, _ = row
    case = cases[0]
    c = Case(ctx, case[0], case[1], case[2] if len(case) > 2 else None, case[3] if len(case) > 3 else None)
    yield
    c.predict(kind)
    yield {"V": c.V, "L": c.L, "mean": c.mean, "var": c.var}


def _run_factor(ctx, blocks, factored):
    X, noise = observation_points(sum(blocks))
    ap = Appender(ctx, X, noise)
    for i, nb in enumerate(blocks):
        ap.add(nb)
        if i < factored:
            assert ap.mat.potrf() == 0
    yield
    assert ap.mat.potrf() == 0
    yield {"L": ap.mat.todense("factor")}


def _run_inverse_diag(ctx):
    ap = _factored(ctx, APP)
    yield
    yield {"inverse_diag": ap.mat.inverse_diag()}


def _run_solve_weights(ctx):
    ap = _factored(ctx, T5)
    r = np.random.default_rng(11).standard_normal(sum(T5))
    yield
    yield {"w": ap.mat.solve_weights(r)}


def _run_potrs(ctx):
    ap = _factored(ctx, T5)
    B = np.random.default_rng(12).standard_normal((sum(T5), 3))
    yield
    yield {"X": ap.mat.potrs(B)}


def table():
    """[(id, options, generator function of ctx)]: the generator sets its problem up, yields, does the measured call, and yields
    the row's own results."""
    rows = [("predict/" + r[0], r[2], lambda ctx, r=r: _run_predict(ctx, r)) for r in ROWS]
    for name, opts in FACTOR:
        for shape, blocks, factored in FACTOR_SHAPES:
            rows.append((f"factor/{name}/{shape}", opts, lambda ctx, b=blocks, f=factored: _run_factor(ctx, b, f)))
    for panel in (128, 512):
        rows.append((f"inverse_diag/panel{panel}", {"inverse_diag_panel": panel}, _run_inverse_diag))
    for resident in (0, 1):
        rows.append((f"solve_weights/resident{resident}", {"trsv_resident": resident}, _run_solve_weights))
    rows.append(("potrs/3rhs", {}, _run_potrs))
    return rows


TABLE = table()


def run_row(ctx, apply, row):
    """One run of the row with profiling on for every slot: (fingerprint, the row's results)."""
    _, opts, make = row
    apply(opts)
    gen = make(ctx)
    next(gen)                                    # the problem is set up: from here on every launch counts
    ctx.profile_enable(True)
    ctx.profile_reset()
    before = routes(ctx)
    results = next(gen)
    after = routes(ctx)
    prof = ctx.profile_get()
    ctx.profile_enable(False)
    slots = {k: {"launches": v["launches"], "flops": v["flops"]} for k, v in prof.items() if v["launches"]}
    return {"slots": slots, "routes": {k: after[k] - before[k] for k in ROUTES}}, results


@pytest.fixture(scope="module")
def ctx():
    from linpde_gp_amd import _engine
    return _engine.default_context()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_fixture_has_exactly_the_rows_of_the_table(golden):
    assert sorted(golden) == sorted(r[0] for r in TABLE)


@pytest.mark.parametrize("row", TABLE, ids=[r[0] for r in TABLE])
def test_schedule_fingerprint(ctx, golden, row):
    with restored(ctx, OPTIONS) as apply:
        got, _ = run_row(ctx, apply, row)
    want = golden[row[0]]
    print(f"\n[{row[0]}] {json.dumps(got, sort_keys=True)}")
    assert got["routes"] == want["routes"], f"{row[0]}: route counters {got['routes']}, recorded {want['routes']}"
    assert sorted(got["slots"]) == sorted(want["slots"]), f"{row[0]}: slots {sorted(got['slots'])}, recorded {sorted(want['slots'])}"
    for k, w in want["slots"].items():
        g = got["slots"][k]
        assert g["launches"] == w["launches"], f"{row[0]}: slot {k}: {g['launches']} launches, recorded {w['launches']}"
        assert abs(g["flops"] - w["flops"]) <= FLOPS_RTOL * abs(w["flops"]), f"{row[0]}: slot {k}: {g['flops']!r} flops, recorded {w['flops']!r}"


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_gpu_schedule_fingerprint.py --write")
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "linpde-gp_amd"))
    from linpde_gp_amd import _engine
    context = _engine.default_context()
    out = {}
    for entry in TABLE:
        with restored(context, OPTIONS) as set_options:
            out[entry[0]], _ = run_row(context, set_options, entry)
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(out)} rows to {GOLDEN}")
