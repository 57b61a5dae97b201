"""CPU restatement of the monotonic alignment search (the published Glow-TTS search that monotonic_align packages,
as include/stts2.h states it for stts_maximum_path), in fp32 with one add and one max per cell, and a brute-force
optimum for small cases.  The tests' reference for the device kernel."""
import itertools

import numpy as np


def mas(value, tx, ty):
    """value [Tx, Ty] (any float) -> int32 path [Tx, Ty]: 1 on the best monotonic path of the top-left tx x ty part."""
    v = np.array(value, dtype=np.float32)
    path = np.zeros(v.shape, np.int32)
    neg = np.float32(-1e9)
    for y in range(ty):
        for x in range(max(0, tx + y - ty), min(tx, y + 1)):
            v_cur = neg if x == y else v[x, y - 1]
            v_prev = (np.float32(0) if y == 0 else neg) if x == 0 else v[x - 1, y - 1]
            v[x, y] = max(v_cur, v_prev) + v[x, y]
    idx = tx - 1
    for y in range(ty - 1, -1, -1):
        path[idx, y] = 1
        if idx != 0 and (idx == y or v[idx, y - 1] < v[idx - 1, y - 1]):
            idx -= 1
    return path


def mas_batch(value, tx, ty):
    return np.stack([mas(value[b], int(tx[b]), int(ty[b])) for b in range(len(value))])


def brute_force(value, tx, ty):
    """The largest sum over all monotonic paths (every column one row, rows 0..tx-1 each at least once), in fp64."""
    best = -np.inf
    for cuts in itertools.combinations(range(1, ty), tx - 1):
        bnd = (0,) + cuts + (ty,)
        best = max(best, sum(float(value[x, bnd[x]:bnd[x + 1]].astype(np.float64).sum()) for x in range(tx)))
    return best
