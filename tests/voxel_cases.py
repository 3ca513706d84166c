"""The VoxelGrid filter at non-finite, signed-zero and far-off points: the clouds, shared by the host check of the
cell arithmetic (tests/test_voxel_cell_host.py) and the GPU test (tests/test_gpu_voxel_values.py), and what the
oracle makes of them.

One point of synth.uniform_cloud(3000, 1.0, 5) is replaced, at index 0, 1500 or 2999.  MUST_FAIL: the Go code
panics (an index out of range, a make() of negative length) or cannot allocate its grid; MUST_PASS: it answers.
Which of the two is never taken from these lists alone: every expectation is the oracle's (expectations()).

The far-off point x = 2e8 asks for a grid of more than 2^32 cells (2e8 / 0.05 = 4e9 per row; chunked, 5e8 chunks
along x times 3 x 3).  The library's contract for such a grid is PCGX_E_OUT_OF_RANGE ("the reference would panic or
need >128 GiB", csrc/voxel_key.h).  The reference does not panic there: it asks the machine for the memory (the
oracle: 36 GB of chunk counters and as much again for its cursors), and an oracle left to itself would answer on a
machine that has it and be killed on one that has not.  So this one verdict is the oracle's in a child process whose
address space is capped at ORACLE_CAP_BYTES = 16 GiB -- below 2^32 x 8 bytes, the least a grid of 2^32 cells costs
it -- and the code it raises is pinned: ORC_E_OOM ("cannot allocate"), where every other failing cloud here is
ORC_E_PANIC (EXPECTED_CODE).  Two ordinary clouds per chunk setting go through the same child and have to come out
as they do in this process."""
import os
import pickle
import subprocess
import sys

import numpy as np

import oracle as O
from pcgol_amd import synth

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N, LEAF = 3000, 0.05
CHUNKS = [(0, 0, 0), (8, 8, 8), (5, 3, 4)]
LAYOUTS = [(12, 0), (16, 0), (15, 1)]
INDICES = [0, 1500, 2999]
ORACLE_CAP_BYTES = 16 << 30

nan, inf = f32(np.nan), f32(np.inf)
KEEP = None  # (this coordinate stays the base cloud's)
MUST_FAIL = {
    "nan_x": (nan, KEEP, KEEP), "nan_y": (KEEP, nan, KEEP), "nan_z": (KEEP, KEEP, nan), "nan_xyz": (nan, nan, nan),
    "+inf_y": (KEEP, inf, KEEP), "-inf_x": (-inf, KEEP, KEEP),
    "+1e30_x": (f32(1e30), KEEP, KEEP), "-1e30_z": (KEEP, KEEP, f32(-1e30)),
    "2e8_x": (f32(2e8), KEEP, KEEP),
}
MUST_PASS = ["1e-45_x", "-0.0_x", "1e-45_xyz", "-0.0_xyz", "vmax_x", "300_copies"]
CAPPED = {"2e8_x"}
EXPECTED_CODE = {name: (O.ORC_E_OOM if name in CAPPED else O.ORC_E_PANIC) for name in MUST_FAIL}


def base_cloud():
    return synth.uniform_cloud(N, 1.0, 5)


def special_cloud(name, index):
    """The base cloud with one point replaced (300_copies: 300 points made copies of one)."""
    pts = base_cloud()
    if name in MUST_FAIL:
        for k, v in enumerate(MUST_FAIL[name]):
            if v is not KEEP:
                pts[index, k] = v
    elif name in ("1e-45_x", "1e-45_xyz", "-0.0_x", "-0.0_xyz"):      # on x alone, and the whole point
        v = f32(1e-45) if name[0] == "1" else f32(-0.0)
        assert v.view(np.uint32) == (1 if name[0] == "1" else 0x80000000)   # the smallest denormal, not a zero; minus zero
        pts[index, : (1 if name.endswith("_x") else 3)] = v
    elif name == "vmax_x":                                  # x == vMax[0] exactly: the last row of the xs stride
        other = [i for i in range(N) if i != index]
        pts[index, 0] = pts[other, 0].max()
    elif name == "300_copies":
        lo = min(index, N - 300)
        pts[lo:lo + 300] = pts[index]
    else:
        raise KeyError(name)
    return pts


def records(pts, stride, off, seed=11):
    """xyz inside records of `stride` bytes at offset `off`, random bytes around them"""
    n = len(pts)
    rec = np.random.default_rng(seed).integers(0, 256, size=(n, stride), dtype=np.uint8)
    rec[:, off:off + 12] = np.ascontiguousarray(pts).view(np.uint8).reshape(n, 12)
    return np.ascontiguousarray(rec)


def oracle_outcome(rec, stride, off, chunk):
    """("raise", code) or ("bytes", the output records) -- in this process"""
    try:
        return ("bytes", O.voxel_filter(rec, N, stride, off, (LEAF,) * 3, chunk))
    except O.OracleError as e:
        return ("raise", e.code)


_CHILD = r"""
import pickle, resource, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import oracle as O
cap = int(sys.argv[2])
resource.setrlimit(resource.RLIMIT_AS, (cap, cap))
out = {}
for key, rec, n, stride, off, leaf, chunk in pickle.load(sys.stdin.buffer):
    try:
        out[key] = ("bytes", O.voxel_filter(rec, n, stride, off, leaf, chunk))
    except O.OracleError as e:
        out[key] = ("raise", e.code)
pickle.dump(out, sys.stdout.buffer)
"""


def capped_expectations(keys):
    """The oracle's outcomes for `keys` = (name, index, chunk, layout), from a child capped at ORACLE_CAP_BYTES (numpy
    and the oracle are all it loads)."""
    O.build()  # (here, not in the child: the compiler is not to run under the cap)
    jobs = [((name, index, chunk, (stride, off)), records(special_cloud(name, index), stride, off), N, stride, off, (LEAF,) * 3, chunk)
            for name, index, chunk, (stride, off) in keys]
    env = dict(os.environ, OPENBLAS_NUM_THREADS="1", OMP_NUM_THREADS="1")
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(ORACLE_CAP_BYTES)], input=pickle.dumps(jobs),
                       stdout=subprocess.PIPE, env=env, check=True)
    return pickle.loads(p.stdout)


def expectations(layouts=LAYOUTS):
    """{(name, index, chunk, layout): ("raise", code) | ("bytes", records)} for every case: the oracle's, in this
    process -- but for the names in CAPPED, whose verdict is the capped child's.  The child is also asked about one
    ordinary failing and one ordinary passing cloud per chunk setting and has to agree with this process on them."""
    keys = [(name, index, chunk, lay) for name in list(MUST_FAIL) + MUST_PASS for index in INDICES for chunk in CHUNKS
            for lay in layouts]
    control = [k for k in keys if k[0] in ("nan_y", "-0.0_x") and k[1] == 1500 and k[3] == layouts[0]]
    capped = capped_expectations([k for k in keys if k[0] in CAPPED] + control)
    exp = {}
    for k in keys:
        name, index, chunk, (stride, off) = k
        if name in CAPPED:
            exp[k] = capped[k]
            continue
        exp[k] = oracle_outcome(records(special_cloud(name, index), stride, off), stride, off, chunk)
    for k in control:
        assert capped[k][0] == exp[k][0] and np.array_equal(capped[k][1], exp[k][1]), k
    return exp
