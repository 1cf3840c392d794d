"""The B-bar products in the flush workgroups of the persistent slice kernel (slice_rider, update.hip) against the form they replace,
the second "chain" of a wrap GEMM (kept behind DQMC_BBAR_RIDER=0).

The rider runs the split-K GEMM's own tile body (gemm_tile.h) on the operands and buffers the wrap piggyback uses, one launch later, so
P, every stack entry, G, log det and the fields are expected BITWISE equal, not close.  The switch is read once per process: each form
computes all cases in one subprocess of its own and leaves them in a file.  That the forms differ is observed, not assumed:
dqmc_bbar_rider_launches counts the slice launches that carried a product, 2 (nt - n_stack) per sweep pair with the rider and 0 without.

Lattices (nt = 12): 8 x 8 (N = 64: F = 4 flush workgroups, 16 tiles, four each), 8 x 10 (N = 80: F = 9, 25 tiles -- an uneven share and a
16-wide edge), 12 x 12 (N = 144: F = 25, 81 tiles), 16 x 16 (N = 256: the kernel instance with literal sizes).  n_stab = 4 (whole blocks)
and n_stab = 5 (blocks of 5, 5 and 2 slices); 8 x 8 also with n_stab = 11, whose last block is ONE slice: loc == 0 is the block's last
slice there, nothing rides and the product stays where it was.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NT = 12
LATTICES = ((8, 8), (8, 10), (12, 12), (16, 16))
N_STABS = (4, 5)
CASES = tuple((L1, L2, ns) for (L1, L2) in LATTICES for ns in N_STABS) + ((8, 8, 11),)
ORACLE_CASES = ((8, 8, 4), (12, 12, 5))
INJECT_CASE = (8, 8, 4)
TOL = 1e-10


def _model(case):
    from dqmc_amd import HubbardModel
    L1, L2, ns = case
    return HubbardModel(L1=L1, L2=L2, U=4.0, beta=1.0, nt=NT, n_stab=ns)


def _inputs(case):
    """seeded i.i.d. fields and the fixed random stream of the sweep pair"""
    m = _model(case)
    rng = np.random.default_rng(1000 + 10 * m.n + case[2])
    return m, m.random_fields(300 + m.n + case[2]), m.random_stream(rng), m.random_stream(rng)


WORKER = r"""
import sys, numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import dqmc_amd
from test_gpu_bbar_rider import _inputs
hip = dqmc_amd.lib()
out = {}
for case in %(cases)r:
    m, f0, sf, sb = _inputs(case)
    key = "%%dx%%d_%%d" %% case
    with m.engine(hip) as e:
        out[key + "_path0"] = np.int64(e.slice_path())
        e.set_fields(f0); e.init()
        for name, sweep, st in (("fwd", e.sweep_0_to_beta, sf), ("bwd", e.sweep_beta_to_0, sb)):
            sweep(*st)
            out[key + "_G_" + name] = e.get_G(); out[key + "_fields_" + name] = e.get_fields()
            out[key + "_acc_" + name] = np.int64(e.stats().n_accepted); out[key + "_ld_" + name] = np.float64(e.get_logdet())
            for i in range(e.n_stack()):
                L, d, R = e.get_stack(i)
                out[key + "_L%%d_" %% i + name] = L; out[key + "_d%%d_" %% i + name] = d; out[key + "_R%%d_" %% i + name] = R
        out[key + "_path1"] = np.int64(e.slice_path()); out[key + "_riders"] = np.int64(e.bbar_rider_launches())
np.savez(sys.argv[1], **out)
print("ok")
"""


def _run(path, cases, env_extra):
    env = dict(os.environ)
    for k in ("DQMC_BBAR_RIDER", "DQMC_DEBUG_SLICE_ABSENT", "DQMC_DEBUG_SLICE_LATE", "DQMC_SLICE_MULTIKERNEL", "DQMC_WALK_SUBMATRIX"):
        env.pop(k, None)
    env.update(env_extra)
    code = WORKER % dict(root=ROOT, tests=os.path.join(ROOT, "tests"), cases=tuple(cases))
    out = subprocess.run([sys.executable, "-c", code, path], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-2000:]
    return dict(np.load(path))


@pytest.fixture(scope="module")
def forms(tmp_path_factory):
    """{name: array} with the rider and with the wrap piggyback: one subprocess each, shared by every case below and never modified"""
    d = tmp_path_factory.mktemp("bbar_rider")
    return _run(str(d / "rider.npz"), CASES, {}), _run(str(d / "piggy.npz"), CASES, {"DQMC_BBAR_RIDER": "0"})


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
    return "%dx%d_%d" % case


def _expected_riders(case):
    """slice launches of one forward and one backward sweep that carry a B-bar product: all but one per block and sweep"""
    return 2 * (NT - -(-NT // case[2]))


def _against_oracle(run, case, oracle_runs):
    fo, Go, acc = oracle_runs[case]
    key = _key(case)
    assert (run[key + "_fields_bwd"] == fo).all(), "HS fields diverged from the oracle"
    assert int(run[key + "_acc_bwd"]) == acc
    err = np.abs(run[key + "_G_bwd"] - Go).max()
    print("%s: max|dG| = %.3e, max|G| = %.3e" % (key, err, np.abs(Go).max()))
    assert err <= TOL * max(1.0, np.abs(Go).max()), err


@pytest.mark.parametrize("case", CASES, ids=_key)
def test_rider_bitwise_equals_wrap_piggyback(forms, case):
    """one forward and one backward sweep: G, the fields, n_accepted, log det and every stack entry after each, the same bits in both
    forms; both forms ran the persistent slice kernel without a fall-back"""
    rider, piggy = forms
    key = _key(case)
    if int(rider[key + "_path0"]) == 0 or int(piggy[key + "_path0"]) == 0:
        pytest.skip("the engine got no CU reservation: no persistent slice kernel, nothing rides")
    for run in (rider, piggy):
        assert int(run[key + "_path0"]) == 1 and int(run[key + "_path1"]) == 1
    # the two forms ARE two forms: every slice but a block's first (forward) / last in walking order (backward) carried a product
    n_stack = -(-NT // case[2])
    assert int(rider[key + "_riders"]) == _expected_riders(case) > 0 and int(piggy[key + "_riders"]) == 0
    skip = (key + "_path", key + "_riders")
    names = sorted(k for k in rider if k.startswith(key + "_") and not k.startswith(skip))
    assert names == sorted(k for k in piggy if k.startswith(key + "_") and not k.startswith(skip))
    assert len(names) == 2 * (4 + 3 * n_stack)
    for name in names:
        a, b = rider[name], piggy[name]
        if a.dtype == np.float64:
            assert np.isfinite(a).all(), name
        assert a.shape == b.shape and bool((_bits(a) == _bits(b)).all()), "%s differs: max|diff| = %.3e" % (name, np.abs(a - b).max())


@pytest.mark.parametrize("case", ORACLE_CASES, ids=_key)
def test_rider_against_the_oracle(forms, oracle_runs, case):
    """rider on, N = 64 and N = 144: fields identical and max|dG| <= 1e-10 max(1, max|G|) after the sweep pair (the bar of test_gpu_parity.py)"""
    rider, _ = forms
    if int(rider[_key(case) + "_path0"]) == 0:
        pytest.skip("the engine got no CU reservation: no persistent slice kernel, nothing rides")
    assert int(rider[_key(case) + "_riders"]) == _expected_riders(case)
    _against_oracle(rider, case, oracle_runs)


@pytest.mark.parametrize("hook", [{"DQMC_DEBUG_SLICE_ABSENT": "2"}, {"DQMC_DEBUG_SLICE_LATE": "2:3000"}], ids=["absent", "late"])
def test_rider_on_the_recoverable_paths(tmp_path, oracle_runs, hook):
    """N = 64 with the rider on and one flush workgroup that never checks in / checks in 3 ms late (the existing hooks of the solo
    fall-back): that workgroup still computes its tiles of P, so the sweep pair ends without an error on the oracle's trajectory"""
    run = _run(str(tmp_path / "inject.npz"), (INJECT_CASE,), hook)
    key = _key(INJECT_CASE)
    if int(run[key + "_path0"]) == 0:
        pytest.skip("the engine got no CU reservation: no persistent slice kernel, nothing rides")
    assert int(run[key + "_path1"]) == 2, "the solo fall-back was not taken"
    assert int(run[key + "_riders"]) == _expected_riders(INJECT_CASE)
    _against_oracle(run, INJECT_CASE, oracle_runs)
