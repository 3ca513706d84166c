"""What one ICP iteration launches (csrc/icp_step_plan.h, plan_step) is what commit 4e440c1 launched.

The header is compiled for the host with g++ (tests/cpp/step_plan_host.cpp; it needs neither HIP nor the library) and
plan_step is compared, field by field, over the full product of its inputs (about 2.4 million cases) with parent_plan()
below: a restatement in numpy of enqueue_corr / enqueue_strict of pcgol_amd/csrc/icp.hip at commit 4e440c1, where the
decision was spread over those two functions and flags parked on the session.  The line numbers beside the expressions
are that file's.  Both sides are total functions: combinations a session never holds are compared like the others.
Where the parent left a function early, the values it did not get to are the ones that launch nothing (false)."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BOOL_FACTS = ("patched", "plane", "min_dist", "has_targets", "grid_enabled", "has_cert", "have_match_caller",
              "caller_had_pairs", "exchange", "spec_walk", "may_speculate")
AXES = dict([(name, (0, 1)) for name in BOOL_FACTS] +
            [("strict", (0, 1, 2)), ("host_iter", (0, 1, 2, 3)), ("grid", (8, 128, 136, 512)),
             ("cert_on", (0, 1)), ("spec_on", (0, 1)), ("fused_from", (0, 2, 3)), ("left_blocks", (128, 8))])
# the rows tests/cpp/step_plan_host.cpp reads and writes
IN_ROWS = ("patched", "plane", "strict", "min_dist", "has_targets", "grid_enabled", "has_cert", "have_match_caller",
           "caller_had_pairs", "exchange", "spec_walk", "host_iter", "may_speculate", "grid",
           "cert_on", "spec_on", "fused_from", "left_blocks")
OUT_ROWS = ("corr", "n_corr", "write_caller", "tile_sums", "grid_has_caller_pairs", "cert", "no_walk", "certify",
            "sums_caller", "have_tile_sums", "first_iter", "next_caller_had_pairs")
PATCHED, WALK, GRID_WALK, GRID, NONE = range(5)  # CorrForm
DEFAULT_KNOBS = dict(cert_on=1, spec_on=1, fused_from=2, left_blocks=128)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("step_plan") / "libstep_plan_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC",
                           "-I" + os.path.join(ROOT, "pcgol_amd", "csrc"), "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "step_plan_host.cpp")])
    return ctypes.CDLL(so)


def plan_step(lib, cases):
    """cases: name -> int array (all IN_ROWS) -> name -> array (OUT_ROWS), from the header"""
    n = len(cases["strict"])
    rows = np.ascontiguousarray(np.stack([np.asarray(cases[k], np.int16) for k in IN_ROWS]))
    out = np.empty((len(OUT_ROWS), n), np.int16)
    lib.step_plan_cases(rows.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(n), out.ctypes.data_as(ctypes.c_void_p))
    return {k: out[i] for i, k in enumerate(OUT_ROWS)}


def parent_plan(c):
    """icp.hip at 4e440c1, enqueue_corr (1080-1205) and enqueue_strict (1207-1246), on arrays"""
    b = {k: np.asarray(c[k]) != 0 for k in BOOL_FACTS + ("cert_on", "spec_on")}
    strict, host_iter, s_grid = (np.asarray(c[k]).astype(np.int64) for k in ("strict", "host_iter", "grid"))
    fused_from, left_blocks = (np.asarray(c[k]).astype(np.int64) for k in ("fused_from", "left_blocks"))
    patched = b["patched"]  # 1084 (the fact is the session's flag after that line); 1090: return, nothing below runs
    live = ~patched
    # 1088: caller_order_fresh = false; 1091: strict == 1 && !plane && nt > 0; 1107: = d_match_caller != nullptr
    caller_order_fresh = live & (strict == 1) & ~b["plane"] & b["has_targets"] & b["have_match_caller"]
    grid = live & b["grid_enabled"] & ~b["min_dist"] & b["has_targets"]  # 1117
    # 1089: false; 1121
    tile_sums_fresh = grid & caller_order_fresh & (strict == 1) & ~b["plane"] & ~b["exchange"]
    # 1126-1127 (a patched step launches s->grid workgroups: 1062-1074)
    n_corr = np.where(grid & (strict != 0) & ~b["plane"] & (s_grid > left_blocks), left_blocks, s_grid)
    cert = grid & b["cert_on"] & b["has_cert"]  # 1128-1129
    no_walk = (live & b["may_speculate"] & b["spec_on"] & b["spec_walk"] & grid & (strict == 1) & ~b["plane"] &
               (host_iter >= 1) & ~tile_sums_fresh)  # 1136-1137
    certify = (no_walk & (fused_from > 0) & (host_iter >= fused_from) & cert & b["caller_had_pairs"] &
               caller_order_fresh & b["exchange"])  # 1085: false; 1148-1149
    # 1090 | 1150: return before any launch | 1151 grid pass, 1175: return | 1151, 1176 | 1176
    corr = np.select([patched, certify, no_walk, grid], [PATCHED, NONE, GRID, GRID_WALK], WALK)
    # 1159 (after 1154: plane), 1166: the strict grid kernel's caller_has_pairs; the others take the default, 0
    grid_has_caller_pairs = grid & (strict != 0) & ~b["plane"] & b["caller_had_pairs"]
    # enqueue_strict 1214-1234: certify -> {match_caller, none}, false (1227-1228);
    # caller_order_fresh -> {match_caller, none}, tile_sums_fresh (1229-1231); else {match, pos_of}, false (1233-1234)
    sums_caller = certify | caller_order_fresh
    have_tile_sums = np.where(certify, False, np.where(caller_order_fresh, tile_sums_fresh, False))
    return {"corr": corr, "n_corr": n_corr,
            "write_caller": caller_order_fresh,  # 1165-1166, 1184-1185
            "tile_sums": tile_sums_fresh,        # 1122, 1186
            "grid_has_caller_pairs": grid_has_caller_pairs, "cert": cert, "no_walk": no_walk, "certify": certify,
            "sums_caller": sums_caller, "have_tile_sums": have_tile_sums,
            "first_iter": host_iter == 0,        # 1213
            "next_caller_had_pairs": caller_order_fresh}  # 1087: what the next enqueue_corr reads


@pytest.fixture(scope="module")
def product():
    names = list(AXES)
    grids = np.meshgrid(*[np.asarray(AXES[k], np.int16) for k in names], indexing="ij")
    return {k: g.ravel() for k, g in zip(names, grids)}


def test_the_whole_input_space_decides_as_the_parent_did(host, product):
    n = len(product["strict"])
    assert n == 2 ** len(BOOL_FACTS) * 3 * 4 * 4 * 2 * 2 * 3 * 2 == 2_359_296
    got, want = plan_step(host, product), parent_plan(product)
    assert set(got) == set(want) == set(OUT_ROWS)
    for k in OUT_ROWS:
        differ = np.flatnonzero(got[k].astype(np.int64) != np.asarray(want[k]).astype(np.int64))
        first = {name: int(product[name][differ[0]]) for name in AXES} if len(differ) else None
        assert len(differ) == 0, "%s differs in %d of %d cases, first at %r" % (k, len(differ), n, first)
    # the enumeration reaches every kind of step (conditions on the cases, not measurements)
    p = got
    count = lambda m: int(np.count_nonzero(m))  # noqa: E731
    for form in (PATCHED, WALK, GRID_WALK, GRID, NONE):
        assert count(p["corr"] == form) > 0, form
    assert count(p["certify"] != 0) > 0
    assert count((p["no_walk"] != 0) & (p["certify"] == 0)) > 0
    assert count((p["tile_sums"] != 0) & (product["exchange"] == 0)) > 0
    assert count(p["tile_sums"] != 0) == count((p["tile_sums"] != 0) & (product["exchange"] == 0))
    assert count((p["n_corr"] == product["left_blocks"]) & (product["grid"] > product["left_blocks"])) > 0
    assert count(p["n_corr"] == product["grid"]) > 0
    assert count((p["sums_caller"] == 0) & (product["strict"] == 1)) > 0   # {match, pos_of}
    assert count((p["sums_caller"] != 0) & (product["strict"] == 1)) > 0   # {match_caller, none}


def test_knob_defaults(host):
    out = (ctypes.c_int32 * 9)()
    host.step_knob_defaults(out)
    # PCGX_ICP_TIGHT, _CHUNKS, _LEFTOVER_BLOCKS, _CERT, _SPEC_WALK, _FUSED_FROM, PCGX_TEST_ICP_FORCE_WALK, _FUSED_SEARCH,
    # _FUSED_GRID_WALK: icp.hip at 4e440c1, 1081, 1126, 1128, 1134, 1147, 1135, 1216, 1217
    assert list(out) == [32, 2, 128, 1, 1, 2, 0, 0, 0]


# ---- the policy in words ---------------------------------------------------------------------------------------------

# a strict (the reference's sums) session on a canonical tree with a grid and certificates, the flagship C4 Fit: 512
# workgroups, the summary kernel exchanges the tile sums itself, pcgx_icp_session_step enqueues (may_speculate)
C4 = dict(patched=0, plane=0, strict=1, min_dist=0, has_targets=1, grid_enabled=1, has_cert=1, have_match_caller=1,
          caller_had_pairs=1, exchange=1, spec_walk=1, host_iter=2, may_speculate=1, grid=512)


def one(lib, **over):
    c = dict(C4, **DEFAULT_KNOBS)
    c.update(over)
    return {k: int(v[0]) for k, v in plan_step(lib, {k: [v] for k, v in c.items()}).items()}


def test_c4_steady_state_is_certified_in_the_summary_kernel(host):
    for it in (2, 3):
        p = one(host, host_iter=it)
        assert p["corr"] == NONE and p["certify"] and p["no_walk"] and p["cert"]
        assert p["sums_caller"] and not p["have_tile_sums"] and not p["first_iter"] and p["next_caller_had_pairs"]


def test_c4_first_iterations(host):
    p = one(host, host_iter=0, caller_had_pairs=0)
    assert p["corr"] == GRID_WALK and p["first_iter"] and not p["no_walk"] and not p["certify"]
    assert p["n_corr"] == 128 and p["write_caller"] and p["sums_caller"] and not p["grid_has_caller_pairs"]
    p = one(host, host_iter=1)  # the second Evaluate: the grid pass alone, on the speculation that it answers every target
    assert p["corr"] == GRID and p["no_walk"] and not p["certify"] and p["grid_has_caller_pairs"]
    assert one(host, host_iter=2, fused_from=3)["corr"] == GRID and one(host, host_iter=3, fused_from=3)["corr"] == NONE
    assert one(host, host_iter=3, fused_from=0)["corr"] == GRID  # (0: never)


def test_a_replay_or_a_session_that_missed_never_speculates(host):
    for it, over in itertools.product((0, 1, 2, 3), (dict(may_speculate=0), dict(spec_walk=0), dict(spec_on=0))):
        p = one(host, host_iter=it, **over)  # settle()'s replay, Evaluate, the sharded step | after a miss | the knob
        assert p["corr"] == GRID_WALK and not p["no_walk"] and not p["certify"], (it, over)


def test_certified_steps_need_certificates_and_last_steps_pairs(host):
    for over in (dict(has_cert=0), dict(cert_on=0), dict(caller_had_pairs=0), dict(have_match_caller=0), dict(exchange=0)):
        p = one(host, **over)
        assert not p["certify"] and p["corr"] in (GRID, GRID_WALK), over
    p = one(host, exchange=0)  # the correspondence kernels form the tile sums: the leftover walk has to run
    assert p["corr"] == GRID_WALK and p["tile_sums"] and p["have_tile_sums"]
    p = one(host, have_match_caller=0)  # no memory for the caller-order pairs: the sums gather through pos_of
    assert not p["write_caller"] and not p["sums_caller"] and not p["next_caller_had_pairs"]


def test_min_dist_never_takes_the_grid(host):
    for strict, it in itertools.product((0, 1, 2), (0, 1, 2, 3)):
        p = one(host, min_dist=1, strict=strict, host_iter=it)
        assert p["corr"] == WALK and p["n_corr"] == 512 and not p["cert"] and not p["no_walk"], (strict, it)


def test_a_patched_tree_takes_nothing_else(host):
    for strict, plane, it in itertools.product((0, 1, 2), (0, 1), (0, 2)):
        p = one(host, patched=1, strict=strict, plane=plane, host_iter=it)
        assert p["corr"] == PATCHED and p["n_corr"] == 512
        assert not any(p[k] for k in OUT_ROWS if k not in ("corr", "n_corr", "first_iter")), (strict, plane, it)


def test_only_strict_sessions_shrink_the_leftover_walk(host):
    assert one(host, strict=0)["n_corr"] == 512 and one(host, strict=2)["n_corr"] == 128
    assert one(host, plane=1, strict=0)["n_corr"] == 512
    assert one(host, grid=128)["n_corr"] == 128 and one(host, grid=136)["n_corr"] == 128
    assert one(host, grid=8, left_blocks=8)["n_corr"] == 8 and one(host, grid=136, left_blocks=8)["n_corr"] == 8
    for strict in (0, 2):  # float64 sums and the one-wave chain: grid pass and walk in every iteration, no caller order
        p = one(host, strict=strict)
        assert p["corr"] == GRID_WALK and not p["write_caller"] and not p["sums_caller"] and p["cert"]
