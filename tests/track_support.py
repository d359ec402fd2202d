"""What the GPU tests of rsik_track share (tests/test_gpu_track.py, tests/test_gpu_track_edges.py): the solvers they launch on, the
seeded inputs of a launch, one launch through HipSolver.track with the results on the host, and the bit comparison of two launches.
torch and the package are imported inside functions.  No test in this file: pytest does not rewrite its asserts, so every one of them
carries its own message."""
import itertools

import numpy as np
import pytest

import arm_pairs
import jacobian_workload as JW
import track_workload as TW
from compare import bits
from gpu_support import T, arm_kwargs

OUTS = ("joints", "rates", "err", "final_joints", "final_err")
NONE, ALL = (), ("ff", "rest", "limits")
CONFIGS = tuple(itertools.product(TW.LAMBDAS, (NONE, ALL)))

_SOLVERS = {}


def solver_of(pair):
    """The pair's solver, uploaded once for the module that runs (the fixture below closes it when that module is done)."""
    if pair not in _SOLVERS:
        _SOLVERS[pair] = arm_pairs.upload(pair, **({"check": lambda p, b: None} if pair == "default/default" else {}))
    return _SOLVERS[pair]


@pytest.fixture(scope="module", autouse=True)
def solvers_do_not_outlive_the_module(torch_mod):
    """(a test module that launches through solver_of imports this fixture by name)"""
    yield
    torch_mod.cuda.synchronize()
    while _SOLVERS:
        _SOLVERS.popitem()[1].close()
    torch_mod.cuda.empty_cache()


def kind_arm(kind, n):
    return {"r": np.zeros(n, dtype=np.uint8), "l": np.ones(n, dtype=np.uint8), "mixed": JW.arm_bytes()[:n]}[kind]


def inputs(pair, n, n_steps, arm, terms):
    """The seeded inputs of a launch on the first n rows: dict of m12 [T,12,n], start [n,7], R, p and the terms' arrays."""
    R, p = TW.goals_of(pair, n_steps, arm)
    d = dict(R=R, p=p, m12=TW.m12_of(R, p), start=TW.starts()[:n], ff=None, rest=None, rest_gain=0.0, limits=None)
    if "ff" in terms:
        d["ff"] = np.ascontiguousarray(TW.feedforwards(n_steps)[:, :n])
    if "rest" in terms:
        d["rest"], d["rest_gain"] = TW.rests()[:n], TW.REST_GAIN
    if "limits" in terms:
        d["limits"] = TW.LIMITS
    return d


def inputs_of(R, p, start, ff=None, rest=None, rest_gain=0.0, limits=None):
    """The inputs of a launch on goals (R [T,n,3,3], p [T,n,3]) and starts of the caller's own, in the form inputs() returns."""
    return dict(R=R, p=p, m12=TW.m12_of(R, p), start=np.ascontiguousarray(start), ff=None if ff is None else np.ascontiguousarray(ff),
                rest=rest, rest_gain=rest_gain, limits=limits)


def launch(torch, pair, kind, arm, d, lam, want=OUTS, dt=TW.DT, kp=TW.KP, ko=TW.KO):
    """One launch through HipSolver.track; lam a float or an array [n]; the results on the host."""
    t = lambda a: None if a is None else T(a, torch)  # noqa: E731
    res = solver_of(pair).track(T(d["m12"], torch), T(d["start"], torch), dt, kp, ko, damping=lam if isinstance(lam, float) else T(lam, torch),
                                feedforward=t(d["ff"]), rest_joints=t(d["rest"]), rest_gain=d["rest_gain"], limits=d["limits"],
                                want=want, **arm_kwargs(kind, arm, torch))
    torch.cuda.synchronize()
    assert tuple(res) == tuple(o for o in OUTS if o in want), (tuple(res), want)
    return {k: a.cpu().numpy() for k, a in res.items()}


def same(a, b, what):
    for k in b:
        assert a[k].shape == b[k].shape and np.array_equal(bits(a[k]), bits(b[k])), (what, k)


def row_alone(d, i):
    """The inputs of trajectory i of a launch's inputs d, as a launch with n = 1."""
    return {k: (a if a is None or k in ("rest_gain", "limits") else np.ascontiguousarray(
        a[:, i:i + 1] if k in ("R", "p", "ff") else a[..., i:i + 1] if k == "m12" else a[i:i + 1])) for k, a in d.items()}
