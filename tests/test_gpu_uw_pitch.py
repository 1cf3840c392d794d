"""The walk's pending-pair store with padded rows (pitch = 1 mod 16, dqmc_amd/csrc/scan_layout.h) on the device.

The padding moves LDS rows and changes no arithmetic.  Every kernel that shares the layout is run on the same inputs: the persistent
slice kernel with the streaming walk, its window-end dump form (DQMC_SLICE_STREAM=0), the scan / flush kernel pairs
(DQMC_SLICE_MULTIKERNEL=1) and the solo fall-back that flushes from the LDS pair store (DQMC_DEBUG_SLICE_ABSENT).  The switches are
read once per process: each setting computes all its cases in one subprocess and leaves them in a file.

Lattices (nt = 12, U = 4, beta = 1, n_stab = 4): 4 x 4 (N = 16: at most 16 pending pairs, the second pivot read is always clamped),
6 x 6 (N = 36: no multiple of 16, pitch 49), 8 x 8 (N = 64), 8 x 10 (N = 80: ragged flush edge) and 16 x 16 (N = 256: the kernel
instance with literal sizes).  Some slice at N >= 64 accepts more than 24 flips, so the rebase copy runs and the second pivot read sees
distinct rows; that is asserted from the per-slice accepted counts.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NT = 12
N_STAB = 4
CASES = ((4, 4), (6, 6), (8, 8), (8, 10), (16, 16))
SOLO_CASE = (8, 8)
SETTINGS = {"persistent": {}, "dump": {"DQMC_SLICE_STREAM": "0"}, "pairs": {"DQMC_SLICE_MULTIKERNEL": "1"}}
EXPECTED_PATH = {"persistent": 1, "dump": 1, "pairs": 0}
HALVES = ("fwd", "bwd")
TOL = 1e-10


def _model(case):
    from dqmc_amd import HubbardModel
    return HubbardModel(L1=case[0], L2=case[1], U=4.0, beta=1.0, nt=NT, n_stab=N_STAB)


def _inputs(case):
    """seeded i.i.d. fields and the fixed random stream of the sweep pair"""
    m = _model(case)
    rng = np.random.default_rng(3100 + 10 * m.n)
    return m, m.random_fields(700 + m.n), m.random_stream(rng), m.random_stream(rng)


WORKER = r"""
import sys, numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import dqmc_amd
from test_gpu_uw_pitch import _inputs
hip = dqmc_amd.lib()
out = {}
for case in %(cases)r:
    m, f0, sf, sb = _inputs(case)
    key = "%%dx%%d" %% case
    with m.engine(hip) as e:
        e.set_fields(f0); e.init()
        for name, sweep, st in (("fwd", e.sweep_0_to_beta, sf), ("bwd", e.sweep_beta_to_0, sb)):
            sweep(*st)
            out[key + "_G_" + name] = e.get_G(); out[key + "_fields_" + name] = e.get_fields()
            out[key + "_acc_" + name] = np.int64(e.stats().n_accepted); out[key + "_ld_" + name] = np.float64(e.get_logdet())
            out[key + "_slices_" + name] = e.debug_snapshot()["accepted"]
        out[key + "_path"] = np.int64(e.slice_path())
np.savez(sys.argv[1], **out)
print("ok")
"""


def _run(path, cases, env_extra):
    env = dict(os.environ)
    for k in ("DQMC_SLICE_STREAM", "DQMC_BBAR_RIDER", "DQMC_DEBUG_SLICE_ABSENT", "DQMC_DEBUG_SLICE_LATE", "DQMC_SLICE_MULTIKERNEL", "DQMC_WALK_SUBMATRIX"):
        env.pop(k, None)
    env.update(env_extra)
    code = WORKER % dict(root=ROOT, tests=os.path.join(ROOT, "tests"), cases=tuple(cases))
    out = subprocess.run([sys.executable, "-c", code, path], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-2000:]
    return dict(np.load(path))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{setting: {name: array}}: one subprocess per switch setting, shared by every test below and never modified"""
    d = tmp_path_factory.mktemp("uw_pitch")
    return {name: _run(str(d / (name + ".npz")), CASES, env) for name, env in SETTINGS.items()}


@pytest.fixture(scope="module")
def oracle_runs(orc):
    """{case: {half: (fields, G, n_accepted)}} of the oracle on the same fields and stream, computed once"""
    res = {}
    for case in CASES:
        m, f0, sf, sb = _inputs(case)
        o = m.engine(orc); o.set_fields(f0); o.init()
        res[case] = {}
        for half, sweep, st in (("fwd", o.sweep_0_to_beta, sf), ("bwd", o.sweep_beta_to_0, sb)):
            sweep(*st)
            res[case][half] = (o.get_fields(), o.get_G(), o.stats().n_accepted)
    return res


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _key(case):
    return "%dx%d" % case


def _against_oracle(run, case, oracle_runs):
    key = _key(case)
    for half in HALVES:
        fo, Go, acc = oracle_runs[case][half]
        assert (run[key + "_fields_" + half] == fo).all(), "HS fields diverged from the oracle (%s)" % half
        assert int(run[key + "_acc_" + half]) == acc
        err = np.abs(run[key + "_G_" + half] - Go).max()
        print("%s %s: max|dG| = %.3e, max|G| = %.3e" % (key, half, err, np.abs(Go).max()))
        assert err <= TOL * max(1.0, np.abs(Go).max()), err


@pytest.mark.parametrize("other", ("dump", "pairs"))
@pytest.mark.parametrize("case", CASES, ids=_key)
def test_paths_bitwise_equal(runs, case, other):
    """forward and backward sweep: the fields, n_accepted, log det, G and the per-slice accepted counts after each half sweep carry the
    same bits on the persistent path and on the other path; every setting ran the path it names without a fall-back"""
    key = _key(case)
    for name in ("persistent", other):
        assert int(runs[name][key + "_path"]) == EXPECTED_PATH[name], name
    a_run, b_run = runs["persistent"], runs[other]
    names = sorted(k for k in a_run if k.startswith(key + "_") and k != key + "_path")
    assert len(names) == 2 * 5 and names == sorted(k for k in b_run if k.startswith(key + "_") and k != key + "_path")
    worst = {}
    for name in names:
        a, b = a_run[name], b_run[name]
        assert a.shape == b.shape
        if a.dtype == np.float64:
            assert np.isfinite(a).all() and np.isfinite(b).all(), name
        if not bool((_bits(a) == _bits(b)).all()):
            worst[name] = float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())
    print("%s persistent vs %s: differing arrays %s" % (key, other, worst))
    assert not worst, worst


@pytest.mark.parametrize("case", CASES, ids=_key)
def test_windows_are_exercised(runs, case):
    """every slice accepts something; at N >= 64 some slice of either sweep accepts more than 24 flips (a publish inside the walk, the
    rebase copy, and k > 17 pending pairs: distinct rows in the second pivot read); at N = 16 no slice can"""
    key = _key(case)
    n = case[0] * case[1]
    for half in HALVES:
        acc = runs["persistent"][key + "_slices_" + half]
        print("%s %s: accepted per slice %s" % (key, half, acc.tolist()))
        assert acc.shape == (NT,) and int(acc.min()) > 0
        if n >= 64:
            assert int(acc.max()) > 24
        if n == 16:
            assert int(acc.max()) <= 16


@pytest.mark.parametrize("setting", tuple(SETTINGS))
@pytest.mark.parametrize("case", CASES, ids=_key)
def test_against_the_oracle(runs, oracle_runs, case, setting):
    """fields identical and max|dG| <= 1e-10 max(1, max|G|) after each half sweep, on every path"""
    _against_oracle(runs[setting], case, oracle_runs)


def test_solo_fall_back_flushes_from_the_padded_store(tmp_path, oracle_runs):
    """N = 64, one flush workgroup never checks in: the walk goes solo (path 2) and applies its windows from the LDS pair store
    (flush_tiles_lds reads the padded rows); the sweep pair stays on the oracle's trajectory"""
    run = _run(str(tmp_path / "absent.npz"), (SOLO_CASE,), {"DQMC_DEBUG_SLICE_ABSENT": "2"})
    assert int(run[_key(SOLO_CASE) + "_path"]) == 2, "the solo fall-back was not taken"
    _against_oracle(run, SOLO_CASE, oracle_runs)
