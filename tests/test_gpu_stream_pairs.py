"""The persistent slice kernel's streaming walk (every accepted pair stored to the ring panels the moment it is formed, update.hip)
against the form it replaces, the window-end dump (kept behind DQMC_SLICE_STREAM=0).

Both forms hand the flush workgroups the same values in the same logical order, so G, the fields, n_accepted, log det and every
stack entry are expected BITWISE equal, not close.  The switch is read once per process: each form computes all cases in one
subprocess of its own and leaves them in a file.

Lattices (nt = 12, U = 4, beta = 1, n_stab = 4): 8 x 8 (N = 64: about 40 accepted flips per slice -- one publish inside the walk and
one at the slice's end, the ring never wraps), 8 x 10 (N = 80: F = 9 flush workgroups, a 16-wide edge), 12 x 12 (N = 144) and
16 x 16 (N = 256, the kernel instance with literal sizes): slices with more than 64 accepted flips, i.e. ring rows that are written a
second time within one launch.  That is asserted from the per-slice accepted counts of dqmc_debug_snapshot, not assumed.
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
CASES = ((8, 8), (8, 10), (12, 12), (16, 16))
WRAP_CASES = ((12, 12), (16, 16))
ORACLE_CASES = ((8, 8), (12, 12))
INJECT_CASE = (8, 8)
RING_ROWS = 64
TOL = 1e-10


def _model(case):
    from dqmc_amd import HubbardModel
    return HubbardModel(L1=case[0], L2=case[1], U=4.0, beta=1.0, nt=NT, n_stab=N_STAB)


def _inputs(case):
    """seeded i.i.d. fields and the fixed random stream of the sweep pair"""
    m = _model(case)
    rng = np.random.default_rng(2000 + 10 * m.n)
    return m, m.random_fields(500 + m.n), m.random_stream(rng), m.random_stream(rng)


WORKER = r"""
import sys, numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import dqmc_amd
from test_gpu_stream_pairs import _inputs
hip = dqmc_amd.lib()
out = {}
for case in %(cases)r:
    m, f0, sf, sb = _inputs(case)
    key = "%%dx%%d" %% case
    with m.engine(hip) as e:
        out[key + "_path0"] = np.int64(e.slice_path())
        e.set_fields(f0); e.init()
        for name, sweep, st in (("fwd", e.sweep_0_to_beta, sf), ("bwd", e.sweep_beta_to_0, sb)):
            sweep(*st)
            out[key + "_G_" + name] = e.get_G(); out[key + "_fields_" + name] = e.get_fields()
            out[key + "_acc_" + name] = np.int64(e.stats().n_accepted); out[key + "_ld_" + name] = np.float64(e.get_logdet())
            out[key + "_slices_" + name] = e.debug_snapshot()["accepted"]
            for i in range(e.n_stack()):
                L, d, R = e.get_stack(i)
                out[key + "_L%%d_" %% i + name] = L; out[key + "_d%%d_" %% i + name] = d; out[key + "_R%%d_" %% i + name] = R
        out[key + "_path1"] = np.int64(e.slice_path())
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
def forms(tmp_path_factory):
    """{name: array} with the streaming walk and with the dump: one subprocess each, shared by every case below and never modified"""
    d = tmp_path_factory.mktemp("stream_pairs")
    return _run(str(d / "stream.npz"), CASES, {}), _run(str(d / "dump.npz"), CASES, {"DQMC_SLICE_STREAM": "0"})


@pytest.fixture(scope="module")
def oracle_runs(orc):
    """{case: (fields, G, n_accepted)} of the oracle after the sweep pair, computed once"""
    res = {}
    for case in set(ORACLE_CASES) | {INJECT_CASE}:
        m, f0, sf, sb = _inputs(case)
        o = m.engine(orc); o.set_fields(f0); o.init(); o.sweep_0_to_beta(*sf); o.sweep_beta_to_0(*sb)
        res[case] = (o.get_fields(), o.get_G(), o.stats().n_accepted)
    return res


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _key(case):
    return "%dx%d" % case


def _against_oracle(run, case, oracle_runs):
    fo, Go, acc = oracle_runs[case]
    key = _key(case)
    assert (run[key + "_fields_bwd"] == fo).all(), "HS fields diverged from the oracle"
    assert int(run[key + "_acc_bwd"]) == acc
    err = np.abs(run[key + "_G_bwd"] - Go).max()
    print("%s: max|dG| = %.3e, max|G| = %.3e" % (key, err, np.abs(Go).max()))
    assert err <= TOL * max(1.0, np.abs(Go).max()), err


@pytest.mark.parametrize("case", CASES, ids=_key)
def test_stream_bitwise_equals_dump(forms, case):
    """one forward and one backward sweep: G, the fields, n_accepted, log det, the per-slice accepted counts and every stack entry after
    each, the same bits in both forms; both forms ran the persistent slice kernel without a fall-back"""
    stream, dump = forms
    key = _key(case)
    for run in (stream, dump):
        assert int(run[key + "_path0"]) == 1 and int(run[key + "_path1"]) == 1
    n_stack = -(-NT // N_STAB)
    names = sorted(k for k in stream if k.startswith(key + "_") and not k.startswith(key + "_path"))
    assert names == sorted(k for k in dump if k.startswith(key + "_") and not k.startswith(key + "_path"))
    assert len(names) == 2 * (5 + 3 * n_stack)
    for name in names:
        a, b = stream[name], dump[name]
        if a.dtype == np.float64:
            assert np.isfinite(a).all(), name
        assert a.shape == b.shape and bool((_bits(a) == _bits(b)).all()), "%s differs: max|diff| = %.3e" % (name, np.abs(a - b).max())


@pytest.mark.parametrize("case", CASES, ids=_key)
def test_ring_wraps_where_it_should(forms, case):
    """N = 144 and N = 256: in either sweep some slice accepts more than 64 flips, so ring rows are rewritten inside one launch;
    N = 64: some slice closes a window inside the walk (more than 24 accepted flips) and none wraps the ring"""
    stream, _ = forms
    key = _key(case)
    for name in ("fwd", "bwd"):
        acc = stream[key + "_slices_" + name]
        print("%s %s: accepted per slice %s" % (key, name, acc.tolist()))
        assert acc.shape == (NT,) and int(acc.min()) > 0
        if case in WRAP_CASES:
            assert int(acc.max()) > RING_ROWS
        if case == (8, 8):
            assert 24 < int(acc.max()) <= RING_ROWS


@pytest.mark.parametrize("case", ORACLE_CASES, ids=_key)
def test_stream_against_the_oracle(forms, oracle_runs, case):
    """streaming walk, N = 64 and N = 144: fields identical and max|dG| <= 1e-10 max(1, max|G|) after the sweep pair"""
    stream, _ = forms
    assert int(stream[_key(case) + "_path0"]) == 1
    _against_oracle(stream, case, oracle_runs)


def test_stream_with_an_absent_flush_workgroup(tmp_path, oracle_runs):
    """N = 64, one flush workgroup never checks in: the walk goes solo (path 2) and applies its windows from LDS while its pair stores go
    on unread; the sweep pair ends on the oracle's trajectory"""
    run = _run(str(tmp_path / "absent.npz"), (INJECT_CASE,), {"DQMC_DEBUG_SLICE_ABSENT": "2"})
    key = _key(INJECT_CASE)
    assert int(run[key + "_path0"]) == 1
    assert int(run[key + "_path1"]) == 2, "the solo fall-back was not taken"
    _against_oracle(run, INJECT_CASE, oracle_runs)
