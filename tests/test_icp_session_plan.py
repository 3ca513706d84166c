"""What an ICP session is and holds (csrc/icp_session_plan.h, plan_session) is what commit 897de71 made it.

The header is compiled for the host with g++ (tests/cpp/session_plan_host.cpp; it needs neither HIP nor the library) and
plan_session is compared, field by field, over the full product of its inputs (368 640 cases) with parent_session()
below: a restatement in numpy of session_create of pcgol_amd/csrc/icp.hip at commit 897de71, where kind, sums, the
one-launch decision and some twenty allocation sizes sat in one function body.  The line numbers beside the expressions
are that file's.  Both sides are total functions: combinations no entry point produces (normals AND covariances) are
compared like the others.  A buffer the parent did not allocate has size 0.

tests/cpp/owned_blocks_host.cpp is the session's way of freeing what it owns (OwnedBlocks, same header) as a
stand-alone program over a stub allocator."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pcgol_amd", "csrc")

STATE_BYTES = 360  # (any value: sizeof(IcpState) is handed in as a fact)
AXES = dict([("normals", (0, 1)), ("covariances", (0, 1)), ("sums_mode", (0, 1, 2)), ("strict_override", (-1, 0, 1, 2)),
             ("nt", (0, 1, 2, 63, 64, 65, 255, 256, 257, 100_000)), ("n_base", (1, 1000)), ("patched", (0, 1)),
             ("has_nan", (0, 1)), ("small_on", (0, 1)), ("small_eligible", (0, 1)), ("small_wants_order", (0, 1)),
             ("grid", (1, 8, 512)), ("num_cu", (1, 256)), ("caller_sums", (0, 1)), ("state_bytes", (STATE_BYTES,))])
IN_ROWS = tuple(AXES)  # the rows tests/cpp/session_plan_host.cpp reads, in its order
FIELDS = ("gicp", "plane", "strict", "strict_explicit", "small", "gicp_grid", "n_sums", "start_values", "nt_pad",
          "small_buffers")
BUFFERS = ("d_xyz", "d_state", "d_partials", "d_pos_of", "d_match", "d_match_cert", "d_first_leaf", "d_walk_list",
           "d_walk_count", "d_sums", "d_match_id", "d_normals", "d_base_cov", "d_target_cov", "d_dropped", "d_valid",
           "d_small_perm")
OUT_ROWS = FIELDS + BUFFERS
SIZEOF_FLOAT4, SIZEOF_FLOAT2 = 16, 8


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("session_plan") / "libsession_plan_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-I" + CSRC, "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "session_plan_host.cpp")])
    lib = ctypes.CDLL(so)
    n_in, n_out = ctypes.c_int32(), ctypes.c_int32()
    assert lib.session_plan_rows(ctypes.byref(n_in), ctypes.byref(n_out)) == len(BUFFERS)
    assert (n_in.value, n_out.value) == (len(IN_ROWS), len(OUT_ROWS))
    return lib


def plan_session(lib, cases):
    """cases: name -> int array (all IN_ROWS) -> name -> array (OUT_ROWS), from the header"""
    n = len(cases["nt"])
    rows = np.ascontiguousarray(np.stack([np.asarray(cases[k], np.int64) for k in IN_ROWS]))
    out = np.empty((len(OUT_ROWS), n), np.int64)
    lib.session_plan_cases(rows.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(n), out.ctypes.data_as(ctypes.c_void_p))
    return {k: out[i] for i, k in enumerate(OUT_ROWS)}


def parent_session(c):
    """icp.hip at 897de71, session_create (1005-1205) and the session's defaults (741-805), on arrays"""
    b = {k: np.asarray(c[k]) != 0 for k in ("normals", "covariances", "patched", "has_nan", "small_on", "small_eligible",
                                            "small_wants_order", "caller_sums")}
    mode, over, nt, nb, s_grid, num_cu, state = (np.asarray(c[k]).astype(np.int64) for k in (
        "sums_mode", "strict_override", "nt", "n_base", "grid", "num_cu", "state_bytes"))
    zero = np.zeros_like(nt)
    gicp = b["covariances"]        # 1041
    plane = b["normals"] | gicp    # 1042
    strict = np.where(plane, 0, np.where(mode == 0, 1, np.where(mode == 1, 0, 2)))  # 1045
    strict_explicit = strict == 2  # 1046
    env = over >= 0                # 1047: PCGX_ICP_STRICT is set; 1048: '1' -> 1, '2' -> 2, anything else 0
    strict = np.where(env, np.where(plane, 0, over), strict)
    strict_explicit = np.where(env, strict != 0, strict_explicit)  # 1049
    g, cap = (nt + 256 - 1) // 256, num_cu * 8                     # 1056 (kGicpBlock: 643)
    gicp_grid = np.where(gicp, np.where(g < 1, 1, np.where(g > cap, cap, g)), 1)  # 1055, 1057; 800: 1
    n_sums = np.where(plane, 30, 10)                               # 801
    n1 = np.where(nt != 0, nt, 1)                                  # nt ? nt : 1
    # 1130-1131 (small_fit_eligible's answer is a fact; where the parent did not ask, it does not matter)
    small = b["small_on"] & (nt > 0) & ~plane & ~b["patched"] & (strict == 1) & ~b["has_nan"] & b["small_eligible"]
    made = small & (nt > 0)        # 1140, 1160
    nt_pad = np.where(made, (nt + 63) & ~np.int64(63), 0)          # 1161; 758: 0
    plane_only = plane & ~gicp     # 1084: if (gicp) ... 1106: else if (plane)
    return {
        "gicp": gicp, "plane": plane, "strict": strict, "strict_explicit": strict_explicit, "small": small,
        "gicp_grid": gicp_grid, "n_sums": n_sums,
        "start_values": ~small,    # 1132-1139: reset_state + general_prepare unless small
        "nt_pad": nt_pad,
        "small_buffers": made,     # 1162, 1164: d_terms, d_small_sync
        "d_xyz": n1 * 12,          # 1065
        "d_state": state,          # 1066
        "d_partials": (s_grid + nt // 256 + 1 + np.where(gicp, gicp_grid, 0)) * n_sums * 8,  # 1067-1069 (kIcpGridBlock: 150)
        "d_pos_of": n1 * 4,        # 1070
        "d_match": n1 * SIZEOF_FLOAT4,  # 1071
        "d_match_cert": n1 * 4,    # 1072
        "d_first_leaf": n1 * 4,    # 1073
        "d_walk_list": n1 * 4,     # 1074
        "d_walk_count": s_grid * 4,     # 1075
        "d_sums": np.where(b["caller_sums"], 0, n_sums * 8),  # 1077-1080
        "d_match_id": np.where(plane, n1 * 4, 0),             # 1086 | 1108
        "d_normals": np.where(plane_only, nb * SIZEOF_FLOAT4, 0),       # 1109
        "d_base_cov": np.where(gicp, nb * 2 * SIZEOF_FLOAT4, 0),        # 1087
        "d_target_cov": np.where(gicp, n1 * 3 * SIZEOF_FLOAT2, 0),      # 1088
        "d_dropped": np.where(gicp, gicp_grid * 4, 0),                  # 1089
        "d_valid": np.where(made, (nt_pad // 64) * 8, zero),            # 1163
        "d_small_perm": np.where(made & b["small_wants_order"], nt * 4, 0),  # 1166
    }


@pytest.fixture(scope="module")
def product():
    names = list(AXES)
    grids = np.meshgrid(*[np.asarray(AXES[k], np.int64) for k in names], indexing="ij")
    return {k: g.ravel() for k, g in zip(names, grids)}


def test_the_whole_input_space_plans_as_the_parent_did(host, product):
    n = len(product["nt"])
    assert n == 2 * 2 * 3 * 4 * 10 * 2 * 2 ** 5 * 3 * 2 * 2 == 368_640
    got, want = plan_session(host, product), parent_session(product)
    assert set(got) == set(want) == set(OUT_ROWS)
    for k in OUT_ROWS:
        differ = np.flatnonzero(got[k] != np.asarray(want[k]).astype(np.int64))
        first = {name: int(product[name][differ[0]]) for name in AXES} if len(differ) else None
        assert len(differ) == 0, "%s differs in %d of %d cases, first at %r" % (k, len(differ), n, first)
    # the enumeration reaches every kind of session (conditions on the cases, not measurements)
    p = got
    count = lambda m: int(np.count_nonzero(m))  # noqa: E731
    for strict in (0, 1, 2):
        assert count((p["strict"] == strict) & (p["plane"] == 0)) > 0
    assert count(p["plane"] & (p["strict"] != 0)) == 0
    assert count(p["small"]) > 0 and count(p["small"] & (p["d_small_perm"] > 0)) > 0
    assert count(p["small"] & (p["d_small_perm"] == 0)) > 0
    assert count(p["small"] & (p["start_values"] != 0)) == 0 and count((p["small"] == 0) & (p["start_values"] == 0)) == 0
    assert count(p["gicp"] & (p["gicp_grid"] == 1)) > 0 and count(p["gicp_grid"] == 8) > 0   # the clamp at one CU
    assert count(p["gicp_grid"] == 391) > 0                                                  # 100 000 targets, 256 CUs
    assert count((p["gicp"] == 0) & (p["gicp_grid"] != 1)) == 0
    assert count(p["d_sums"] == 0) > 0 and count(p["d_sums"] == 80) > 0 and count(p["d_sums"] == 240) > 0
    assert count((p["d_normals"] > 0) & (p["d_base_cov"] > 0)) == 0


def test_block_sizes_are_the_parents(host):
    out = (ctypes.c_int32 * 2)()
    host.session_block_sizes(out)
    assert list(out) == [256, 256]  # icp.hip at 897de71: kIcpGridBlock (150), kGicpBlock (643)


# ---- rows a reader can check by eye ----------------------------------------------------------------------------------

def one(lib, **facts):
    c = dict(normals=0, covariances=0, sums_mode=0, strict_override=-1, nt=1000, n_base=1000, patched=0, has_nan=0,
             small_on=1, small_eligible=0, small_wants_order=0, grid=1, num_cu=256, caller_sums=0, state_bytes=400)
    c.update(facts)
    return {k: int(v[0]) for k, v in plan_session(lib, {k: [v] for k, v in c.items()}).items()}


def test_the_default_session_on_a_small_cloud_is_one_launch(host):
    p = one(host, nt=1000, n_base=1000, small_eligible=1, grid=4)
    assert p == dict(gicp=0, plane=0, strict=1, strict_explicit=0, small=1, gicp_grid=1, n_sums=10, start_values=0,
                     nt_pad=1024, small_buffers=1, d_xyz=12000, d_state=400, d_partials=(4 + 3 + 1) * 10 * 8,
                     d_pos_of=4000, d_match=16000, d_match_cert=4000, d_first_leaf=4000, d_walk_list=4000, d_walk_count=16,
                     d_sums=80, d_match_id=0, d_normals=0, d_base_cov=0, d_target_cov=0, d_dropped=0, d_valid=16 * 8,
                     d_small_perm=0)
    assert one(host, nt=4000, small_eligible=1, small_wants_order=1)["d_small_perm"] == 16000
    for off in (dict(small_on=0), dict(patched=1), dict(has_nan=1), dict(sums_mode=1), dict(sums_mode=2),
                dict(strict_override=0), dict(small_eligible=0), dict(nt=0)):
        p = one(host, **dict(dict(small_eligible=1), **off))
        assert not p["small"] and p["start_values"] and not p["small_buffers"] and p["d_valid"] == 0 and p["nt_pad"] == 0, off


def test_a_plane_session(host):
    p = one(host, normals=1, nt=5000, n_base=2000, grid=8, small_eligible=1)
    assert p == dict(gicp=0, plane=1, strict=0, strict_explicit=0, small=0, gicp_grid=1, n_sums=30, start_values=1,
                     nt_pad=0, small_buffers=0, d_xyz=60000, d_state=400, d_partials=(8 + 19 + 1) * 30 * 8,
                     d_pos_of=20000, d_match=80000, d_match_cert=20000, d_first_leaf=20000, d_walk_list=20000,
                     d_walk_count=32, d_sums=240, d_match_id=20000, d_normals=2000 * 16, d_base_cov=0, d_target_cov=0,
                     d_dropped=0, d_valid=0, d_small_perm=0)
    assert one(host, normals=1, strict_override=1)["strict"] == 0  # no reference sums to reproduce
    assert one(host, normals=1, caller_sums=1)["d_sums"] == 0


def test_a_gicp_session_at_257_targets(host):
    p = one(host, covariances=1, nt=257, n_base=1000, grid=1)
    assert p == dict(gicp=1, plane=1, strict=0, strict_explicit=0, small=0, gicp_grid=2, n_sums=30, start_values=1,
                     nt_pad=0, small_buffers=0, d_xyz=3084, d_state=400, d_partials=(1 + 1 + 1 + 2) * 30 * 8,
                     d_pos_of=1028, d_match=4112, d_match_cert=1028, d_first_leaf=1028, d_walk_list=1028,
                     d_walk_count=4, d_sums=240, d_match_id=1028, d_normals=0, d_base_cov=1000 * 32,
                     d_target_cov=257 * 24, d_dropped=8, d_valid=0, d_small_perm=0)
    assert one(host, covariances=1, nt=256)["gicp_grid"] == 1 and one(host, covariances=1, nt=0)["gicp_grid"] == 1
    assert one(host, covariances=1, nt=100_000, num_cu=1)["gicp_grid"] == 8


def test_the_sums_a_session_forms(host):
    assert [one(host, sums_mode=m)["strict"] for m in (0, 1, 2)] == [1, 0, 2]
    assert [one(host, sums_mode=m)["strict_explicit"] for m in (0, 1, 2)] == [0, 0, 1]
    for mode in (0, 1, 2):  # PCGX_ICP_STRICT overrides sums_mode, and is asking by name
        assert [one(host, sums_mode=mode, strict_override=o)["strict"] for o in (0, 1, 2)] == [0, 1, 2]
        assert [one(host, sums_mode=mode, strict_override=o)["strict_explicit"] for o in (0, 1, 2)] == [0, 1, 1]


# ---- what a session owns is freed once -------------------------------------------------------------------------------

def test_owned_blocks_over_a_stub_allocator(tmp_path):
    exe = str(tmp_path / "owned_blocks_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I" + CSRC, "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "owned_blocks_host.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")
