"""The option table of the library (csrc/options.cpp): defaults, get / set round trips, refusals and the environment, on
the CPU box.  Like test_host_asan.py it builds the AddressSanitizer library of the host-only code (`build.sh --host-asan`)
and drives it in a subprocess with libasan preloaded (tests/_host_options_worker.py); one subprocess per environment."""
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "linpde-gp_amd", "csrc")
LIB = os.path.join(CSRC, "hosttest", "liblpgp_hosttest_asan.so")

# every row and its default, as the context had them before the table (lpgp_ctx's initialisers, LPGP_RESERVE_CUS's 32);
# doubles read truncated
DEFAULTS = {
    "reserve_cus": 32, "reserve_narrow": 64, "single_stream": 0,
    "nb": 512, "lookahead": 1, "nb_outer": 2048, "nb_outer_min_tiles": 192, "nb_big": 0, "nb_big_min_tiles": 96,
    "chain_us_tile": 150, "chain_us_fixed": 80, "chain_resident_max_rows": 32, "chain_resident2_max_rows": 0, "chain_ahead": 1,
    "chain_ahead_min_rows": 12, "append_split": 0, "append_split_min_tiles": 16,
    "nb_solve": 0, "nb_outer_solve": 4096, "nb_outer_solve_min_tiles": 384, "solve_chain_us_tile": 30, "fused_solve": 1,
    "fused_ahead": 1, "fused_ahead_min_us": 800, "panel_exclusive": 1, "trsv_resident": 1,
    "ride_stream": 57, "ride_occ3": 1, "ride_aug": 0, "ride_b_on_ride": 0, "ride_old_ungated": 1, "ride_vchain_pre": 1,
    "ride_vchain_max_wgs": 96, "ride_gate_pct": -1, "ride_outer_rows": 2048, "ride_outer_min_tiles": 64, "ride_max_tiles": 384,
    "ride_same_stream_max_tiles": 0,
    "gemm3": 768, "gemm3_fact": 0, "gemm3_margin": 2, "small_tiles_max": 256, "small_ring2": 32, "min_supertiles": 128,
    "dense_tiles": 1, "gemm_band": 8,
    "asm_fast": 1, "asm_ct": 4, "asm_batch": 1, "asm_factors": 0, "kron_wide": 1,
    "dist_bcast": 0, "split_gather": 1, "scoped_gather": 1, "dist_chain_us_comm": 120,
}
INIT_ONLY = ("reserve_cus", "reserve_narrow", "single_stream")
BOOLS = ("lookahead", "dense_tiles", "fused_solve", "trsv_resident", "chain_ahead", "ride_occ3", "ride_b_on_ride", "ride_old_ungated",
         "ride_vchain_pre", "append_split", "panel_exclusive", "gemm3_fact", "asm_fast", "asm_factors", "asm_batch", "kron_wide",
         "split_gather", "scoped_gather", "dist_bcast", "single_stream")
SETTABLE = [k for k in DEFAULTS if k not in INIT_ONLY]


@pytest.fixture(scope="module")
def run():
    gxx = shutil.which(os.environ.get("CXX", "g++"))
    if gxx is None:
        pytest.skip("no host C++ compiler")
    libasan = subprocess.run([gxx, "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(libasan) or not os.path.exists(libasan):
        pytest.skip("libasan.so not found")
    subprocess.run(["bash", os.path.join(CSRC, "build.sh"), "--host-asan"], check=True, capture_output=True)
    # the caller's own LPGP_* settings must not leak into the scenarios
    base = {k: v for k, v in os.environ.items() if not k.startswith("LPGP_") and k != "ROCPROF_COUNTER_COLLECTION"}
    base.update(LD_PRELOAD=libasan, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:halt_on_error=1",
                UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")

    def run(env=None, ops=()):
        res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_host_options_worker.py"), LIB, json.dumps(list(ops))],
                             env=dict(base, **(env or {})), capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stdout[-2000:] + "\n" + res.stderr[-4000:]
        assert "ERROR: AddressSanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr[-4000:]
        return json.loads(res.stdout.strip().splitlines()[-1])
    return run


def test_every_row_has_its_default(run):
    rows = run()["rows"]
    assert rows == DEFAULTS
    assert set(BOOLS) <= set(rows)


def test_every_settable_row_round_trips(run):
    ops = [op for k in SETTABLE for op in (["get", k], ["set", k, DEFAULTS[k]])]
    out = run(ops=ops)["ops"]
    for i, k in enumerate(SETTABLE):
        assert out[2 * i] == [0, DEFAULTS[k]], k
        assert out[2 * i + 1] == [0, DEFAULTS[k]], k


def test_rows_are_stored_apart(run):
    """Every settable row set to a value other than its default; every row then reads its own value (no two rows share
    storage, no store spills into a neighbour)."""
    special = {"nb": 1024, "nb_outer": 2560, "nb_big": 512, "nb_solve": 256, "nb_outer_solve": 384, "ride_outer_rows": 1024,
               "asm_ct": 9, "gemm_band": 16, "nb_outer_solve_min_tiles": 7}
    want = {k: special.get(k, 1 - DEFAULTS[k] if k in BOOLS else DEFAULTS[k] + 3 + i) for i, k in enumerate(SETTABLE)}
    ops = [["set", k, v] for k, v in want.items()] + [["get", k] for k in DEFAULTS]
    out = run(ops=ops)["ops"]
    assert all(rc == 0 for rc, _ in out), out
    got = {k: v for k, (_, v) in zip(DEFAULTS, out[len(want):])}
    assert got == dict(DEFAULTS, **want)


@pytest.mark.parametrize("key,value,message", [
    ("nb", 100, "nb must be a positive multiple of 128"),
    ("nb", 0, "nb must be a positive multiple of 128"),
    ("nb_solve", 100, "nb_solve must be a multiple of 128 (0: nb)"),
    ("nb_outer", 100, "nb_outer must be a multiple of 128 (0 disables)"),
    ("nb_outer_solve", -128, "nb_outer_solve must be a multiple of 128 (0 disables)"),
    ("nb_big", 100, "nb_big must be a multiple of 128 (0 disables)"),
    ("ride_outer_rows", 256, "ride_outer_rows must be a multiple of 512 (0 disables)"),
    ("asm_ct", 0, "asm_ct must be in 1 .. 64"),
    ("asm_ct", 65, "asm_ct must be in 1 .. 64"),
    ("nb_outer_solve_min_tiles", -1, "nb_outer_solve_min_tiles must be >= 0"),
    ("gemm_band", 3, "gemm_band must be one of 2, 4, 8, 16, 32"),
    ("no_such_option", 1, "unknown option no_such_option"),
])
def test_refused_values_keep_the_old_one(run, key, value, message):
    out = run(ops=[["set", key, value], ["get", key]])["ops"]
    assert out[0] == [-2, message]
    if key in DEFAULTS:
        assert out[1] == [0, DEFAULTS[key]]
    else:
        assert out[1] == [-2, message]


def test_special_rows(run):
    out = run(ops=[["set", "gemm3", 5], ["set", "gemm3", -1], ["set", "gemm3", 0],
                   ["set", "trsv_resident", 2], ["set", "dense_tiles", -3], ["set", "ride_aug", 2],
                   ["set", "chain_us_tile", 99], ["set", "gemm_band", 32], ["set", "ride_gate_pct", -1]]
              + [["set", k, 0] for k in INIT_ONLY])["ops"]
    assert out[:9] == [[0, 5], [0, 768], [0, 0], [0, 1], [0, 1], [0, 2], [0, 99], [0, 32], [0, -1]]
    for (rc, msg), k in zip(out[9:], INIT_ONLY):
        assert rc == -2 and msg.startswith(f"{k} is read at lpgp_init only"), msg


@pytest.mark.parametrize("env,key,value", [
    ({"LPGP_NB": "100"}, "nb", 512),
    ({"LPGP_NB": "256"}, "nb", 256),
    ({"LPGP_GEMM_BAND": "3"}, "gemm_band", 8),
    ({"LPGP_GEMM_BAND": "16"}, "gemm_band", 16),
    ({"LPGP_TRSV_RESIDENT": "2"}, "trsv_resident", 1),
    ({"LPGP_CHAIN_US_TILE": "99.7"}, "chain_us_tile", 99),
    ({"LPGP_DIST_COLLECTIVE": "bcast"}, "dist_bcast", 1),
    ({"LPGP_DIST_COLLECTIVE": "p2p"}, "dist_bcast", 0),
    ({"ROCPROF_COUNTER_COLLECTION": "1"}, "ride_vchain_max_wgs", 0),
    ({"ROCPROF_COUNTER_COLLECTION": "0"}, "ride_vchain_max_wgs", 96),
    ({"ROCPROF_COUNTER_COLLECTION": "1", "LPGP_RIDE_VCHAIN": "5"}, "ride_vchain_max_wgs", 5),
    ({"LPGP_RESERVE_CUS": "0"}, "reserve_cus", 0),
    ({"LPGP_RESERVE_CUS_NARROW": "16"}, "reserve_narrow", 16),
    ({"LPGP_SINGLE_STREAM": "1"}, "single_stream", 1),
    ({"LPGP_NB_OUTER_SOLVE": "2048"}, "nb_outer_solve", 2048),
    ({"LPGP_RIDE_GATE_PCT": "65"}, "ride_gate_pct", 65),
    # values the rows refuse are ignored, as they always were for LPGP_NB* and LPGP_GEMM_BAND
    ({"LPGP_ASM_CT": "0"}, "asm_ct", 4),
    ({"LPGP_ASM_CT": "65"}, "asm_ct", 4),
    ({"LPGP_RIDE_OUTER_ROWS": "256"}, "ride_outer_rows", 2048),
    ({"LPGP_NB_OUTER_SOLVE_MIN_TILES": "-1"}, "nb_outer_solve_min_tiles", 384),
])
def test_environment(run, env, key, value):
    rows = run(env)["rows"]
    assert rows == dict(DEFAULTS, **{key: value})
