"""CPU-side checks of rsik_reach_map: declared, exported, bound, ABI version still 8, the Python surface exists, the argument check
that needs no device — and the expected-value helper of the GPU tests (tests/reach_map_workload.py) pinned on the checker alone,
with the conditions the named test grid must meet for tests/test_gpu_reach_map.py to mean something."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from arm_pairs import checker_arms
from compare import bits
from oracle import oracle as orc
from reach_map_workload import N_STATES, expected_map, map_case, pack_mask, rounding_bound, tile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("default/default", "r"), ("default/default", "l"), ("default/default", "mixed"), ("custom/custom", "mixed"),
         ("custom/default", "mixed"), ("default/ztip", "mixed")]


def arms_of(pair):
    return (orc.Arm("r_arm", 0.03), orc.Arm("l_arm", 0.03)) if pair == "default/default" else checker_arms(pair)


def uniform_or_bytes(kind, arm_ids):
    return arm_ids if kind == "mixed" else int(kind == "l")


def test_reach_map_entry_point_is_part_of_abi_8():
    from reachy2_symbolic_ik_amd import _abi

    L = _abi.load()
    assert _abi.ABI_VERSION == 8 == L.rsik_abi_version()
    assert "rsik_reach_map" in _abi.PROTOTYPES
    assert isinstance(L.rsik_reach_map, C._CFuncPtr)
    hdr = open(os.path.join(ROOT, "include", "rsik.h")).read()
    assert "#define RSIK_ABI_VERSION 8" in hdr
    decl = re.search(r"int rsik_reach_map\(([^;]*)\);", hdr)
    assert decl, "include/rsik.h does not declare rsik_reach_map"
    assert len(decl.group(1).split(",")) == len(_abi.PROTOTYPES["rsik_reach_map"][1]) == 11
    assert "within ABI version 8" in hdr
    assert int(re.search(r"#define RSIK_REACH_MAP_STATES (\d+)", hdr).group(1)) == N_STATES
    assert int(re.search(r"#define RSIK_OPT_COUNT (\d+)", hdr).group(1)) == 9
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`rsik_reach_map`" in doc


def test_reach_map_entry_point_refuses_a_null_context():
    from reachy2_symbolic_ik_amd import _abi

    L = _abi.load()
    assert L.rsik_reach_map(None, 0, None, None, 0, 1, None, None, None, None, None) == _abi.RSIK_E_INVALID


def test_python_surface_exists():
    from reachy2_symbolic_ik_amd import DualArmIK, HipSolver, SymbolicIK
    from reachy2_symbolic_ik_amd.symbolic_ik import unpack_reach_mask

    for cls, name in ((HipSolver, "reach_map"), (SymbolicIK, "reach_map_batch"), (DualArmIK, "reach_map_batch")):
        fn = getattr(cls, name)
        assert callable(fn) and "state_count" in fn.__doc__ and "per position" in fn.__doc__.lower(), (cls.__name__, name)
    assert callable(unpack_reach_mask)


def test_mask_helper_round_trip():
    """pack_mask (the tests' NumPy packing) and unpack_reach_mask (the package's torch helper) are each other's inverse, and the
    padding bits are 0."""
    import torch

    from reachy2_symbolic_ik_amd.symbolic_ik import unpack_reach_mask

    for n_rot in (1, 63, 64, 65, 130):
        flags = np.random.default_rng(n_rot).integers(0, 2, size=(5, n_rot)).astype(bool)
        flags[0] = True
        words = pack_mask(flags)
        assert words.dtype == np.uint64 and words.shape == (5, (n_rot + 63) // 64)
        for i in range(5):
            for j in range(n_rot):
                assert bool((int(words[i, j // 64]) >> (j % 64)) & 1) == bool(flags[i, j])
        if n_rot % 64:
            assert int(words[0, -1]) >> (n_rot % 64) == 0
        back = unpack_reach_mask(torch.as_tensor(words.view(np.int64)), n_rot).numpy()
        assert back.dtype == bool and np.array_equal(back, flags)


@pytest.mark.parametrize("pair,kind", [("default/default", "mixed"), ("custom/default", "mixed")])
def test_expected_map_is_a_fresh_is_reachable_per_pose(pair, kind):
    """tests/reach_map_workload.expected_map against the checker's solver OBJECT on a 40-position x 9-orientation subset of the test
    grid: every cell's flag, state and width bits are those of a new orc.Solver's is_reachable; the reductions are recounted here."""
    arms = arms_of(pair)
    P, arm_ids, E = map_case(arms, kind)
    rows = np.random.default_rng(5).choice(len(P), size=40, replace=False)
    P, arm_ids, E = P[rows], arm_ids[rows], E[:9]
    ref = expected_map(orc, arms, P, arm_ids, E)
    assert ref["count"].shape == (40,) and ref["state_count"].shape == (40, N_STATES) and ref["mask"].shape == (40, 1)
    n_ok = 0
    for i in range(40):
        ws, counts = [], np.zeros(N_STATES, dtype=np.int64)
        for j in range(9):
            ok, itv, st = orc.Solver(arms[int(arm_ids[i])]).is_reachable(P[i], E[j])
            assert ok == bool(ref["reachable"][i, j]) and st == ref["state"][i, j], (i, j)
            assert bool((int(ref["mask"][i, 0]) >> j) & 1) == ok
            counts[st] += 1
            w = 0.0
            if ok:
                w = itv[1] - itv[0]
                if itv[0] > itv[1]:
                    w += 2 * math.pi
                assert w > 0.0
            assert bits(w) == bits(ref["width"][i, j]), (i, j)
            ws.append(w)
            n_ok += ok
        assert np.array_equal(counts, ref["state_count"][i]) and counts.sum() == 9
        assert ref["count"][i] == sum(1 for w in ws if w != 0.0)
        assert bits(math.fsum(ws)) == bits(ref["theta_measure"][i])
        assert int(ref["mask"][i, 0]) >> 9 == 0
    assert 40 <= n_ok <= 320


@pytest.mark.parametrize("pair,kind", CASES)
def test_the_test_grid_exercises_the_reduction(pair, kind):
    """n_rot = 130, seed 7, on the checker alone: at least a third of the 729 voxels are mixed (neither all nor none of their
    orientations reachable), at least a third of the 64-orientation chunks are mixed, at least 100 voxels have a reachable orientation
    among the last two (the ragged chunk), at least 100 voxels show three or more state codes, and no reachable pose has
    |i0 - i1| < 1e-6, so the width is continuous in the interval's ends."""
    arms = arms_of(pair)
    P, arm_ids, E = map_case(arms, kind)
    assert P.shape == (729, 3) and E.shape == (130, 3)
    pos, eul, arm = tile(P, uniform_or_bytes(kind, arm_ids), E)
    raw = orc.solve_batch(arms[0], arms[1], pos, eul, arm_id=arm, theta_policy=3, nthreads=4)
    ref = expected_map(orc, arms, P, uniform_or_bytes(kind, arm_ids), E, nthreads=4)
    ok = ref["reachable"]
    mixed_voxels = int(((ref["count"] > 0) & (ref["count"] < 130)).sum())
    chunks = [ok[:, 0:64], ok[:, 64:128]]  # the two full chunks of every voxel: 1458 in all
    mixed_chunks = sum(int(((c.sum(axis=1) > 0) & (c.sum(axis=1) < c.shape[1])).sum()) for c in chunks)
    ragged = int(ok[:, 128:130].any(axis=1).sum())
    codes = int(((ref["state_count"] > 0).sum(axis=1) >= 3).sum())
    itv = raw["interval"][raw["reachable"].astype(bool)]
    gap = float(np.abs(itv[:, 0] - itv[:, 1]).min())
    print(f"{pair} {kind}: {mixed_voxels} mixed voxels, {mixed_chunks} of 1458 mixed full chunks, {ragged} voxels reachable in the ragged "
          f"tail, {codes} voxels with >= 3 codes, min |i0 - i1| {gap:.3e}, states present {np.flatnonzero(ref['state_count'].sum(axis=0))}")
    assert mixed_voxels >= 243
    assert mixed_chunks >= 486
    assert ragged >= 100
    assert codes >= 100
    assert gap >= 1e-6
    assert (ref["state_count"].sum(axis=1) == 130).all()
    # position-only outcomes: whole voxels in one bin
    assert int((ref["state_count"][:, 1] == 130).sum()) + int((ref["state_count"][:, 2] == 130).sum()) >= 81
    assert rounding_bound(130) < 2e-9  # well inside the checker comparison's 2 * TOL per reachable pose
