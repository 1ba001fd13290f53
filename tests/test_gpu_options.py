"""Options on a real context: every key lpgp_get_option / lpgp_set_option accepted before the option table (csrc/options.cpp)
still reads / sets, the read-only state reads 0 on a fresh context, and the environment reaches the context.  One
subprocess per environment (lpgp_init reads it once)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the keys of the per-key branches the table replaced
GET_KEYS = [
    "nb", "gemm3", "gemm3_fact", "dist_bcast", "split_gather", "scoped_gather", "lookahead", "fused_solve", "small_tiles_max",
    "live_mats", "asm_ct", "asm_batch", "kron_wide", "asm_fast", "fused_ahead", "fused_ahead_min_us", "nb_outer_solve",
    "nb_outer_solve_min_tiles", "nb_solve", "solve_chain_us_tile", "chain_us_fixed", "ride_stream", "chain_resident_max_rows",
    "trsv_resident", "chain_resident2_max_rows", "chain_ahead", "chain_ahead_min_rows", "ride_vchain_max_wgs", "ride_occ3", "ride_aug",
    "append_split", "ride_gate_pct", "ride_outer_rows", "ride_outer_min_tiles", "ride_max_tiles", "ride_same_stream_max_tiles",
    "dense_tiles", "min_supertiles", "small_ring2", "nb_outer", "nb_outer_min_tiles", "nb_big", "nb_big_min_tiles",
    "route_ride_done", "route_ride_aug", "route_ride_b2b", "route_ride", "route_ride_vchain", "route_ride_two", "route_ride_outer",
    "route_solve_two_level", "route_solve_ahead", "route_solve_tiles",
]
SET_KEYS = [
    "nb", "small_tiles_max", "chain_us_tile", "solve_chain_us_tile", "chain_us_fixed", "dense_tiles", "fused_solve", "dist_bcast",
    "split_gather", "scoped_gather", "asm_factors", "asm_fast", "asm_batch", "kron_wide", "asm_ct", "gemm3_fact", "gemm3",
    "small_ring2", "fused_ahead", "fused_ahead_min_us", "min_supertiles", "nb_solve", "nb_outer_solve", "nb_outer_solve_min_tiles",
    "nb_outer", "nb_outer_min_tiles", "nb_big", "nb_big_min_tiles", "lookahead", "ride_stream", "chain_resident_max_rows",
    "trsv_resident", "chain_resident2_max_rows", "chain_ahead", "chain_ahead_min_rows", "ride_vchain_max_wgs", "ride_occ3", "ride_aug",
    "append_split", "ride_gate_pct", "ride_outer_rows", "ride_outer_min_tiles", "ride_max_tiles", "ride_same_stream_max_tiles",
]
STATE_KEYS = [k for k in GET_KEYS if k == "live_mats" or k.startswith("route_")]

SCRIPT = r"""
import json, os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "linpde-gp_amd"))
from linpde_gp_amd import _engine
ctx = _engine.Context()
get_keys, set_keys = json.loads(sys.argv[1]), json.loads(sys.argv[2])
got = {k: ctx.get_option(k) for k in get_keys}
for k in set_keys:                      # each set to the value it reads: every key is accepted and the context stays as it was
    v = ctx.get_option(k)
    ctx.set_option(k, v)
    assert ctx.get_option(k) == v, k
ctx.close()
print("OPTIONS " + json.dumps(got))
"""


def run(env, get_keys, set_keys=()):
    base = {k: v for k, v in os.environ.items() if not k.startswith("LPGP_") and k != "ROCPROF_COUNTER_COLLECTION"}
    out = subprocess.run([sys.executable, "-c", SCRIPT % {"root": ROOT}, json.dumps(get_keys), json.dumps(list(set_keys))],
                         env=dict(base, **env), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("OPTIONS ")][-1]
    return json.loads(line[len("OPTIONS "):])


@pytest.mark.gpu
def test_every_former_key_reads_and_sets():
    assert len(GET_KEYS) == 53 and len(SET_KEYS) == 44
    got = run({}, GET_KEYS, SET_KEYS)
    assert set(got) == set(GET_KEYS)
    assert all(got[k] == 0 for k in STATE_KEYS), {k: got[k] for k in STATE_KEYS}
    assert got["nb"] == 512 and got["nb_outer_solve"] == 4096 and got["gemm3"] == 768


@pytest.mark.gpu
def test_environment_reaches_the_context():
    got = run({"LPGP_NB": "256", "LPGP_RESERVE_CUS": "0"}, ["nb", "reserve_cus", "reserve_narrow"])
    assert got == {"nb": 256, "reserve_cus": 0, "reserve_narrow": 64}
