"""The one-launch-per-panel form of the Gauss-Jordan solve (gj_step_kernel, lu_gj.hip) against the two-launch form it replaces
(gj_panel_mw_kernel + gj_update_kernel, kept behind DQMC_GJ_FUSED=0; =1 takes the fused step wherever it has an instance).

Every workgroup of the fused step factors the panel with the device functions the panel kernel uses, and its update keeps the operand
partition of the MFMAs, the order of the six substitution products and the final cold - acc, so G and log det are expected BITWISE
equal, not close.  The switches are read once per process: each form computes all cases in one subprocess of its own and leaves them
in a file.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# 72: tail panel of 8 columns, two waves of rows; 100: tail of 4, odd tile counts; 144: three waves; 256: the flagship instance, 8 full
# panels; 272: above the fused step's largest instance -- the two-launch form in both processes
SIZES = (72, 100, 144, 256, 272)
SEQ_SIZES = (72, 100)
CHAINS = 3

WORKER = r"""
import sys, numpy as np
sys.path.insert(0, %(root)r)
import dqmc_amd
from dqmc_amd.abi import DqmcError
hip = dqmc_amd.lib()
def factor(rng, n):            # scripts/gj_probe.py: orthogonal L, d graded over e^+-8, unit upper R
    Q = np.linalg.qr(rng.standard_normal((n, n)))[0]
    d = np.exp(np.sort(rng.uniform(-8, 8, n))[::-1])
    R = np.triu(rng.standard_normal((n, n)) * 0.2, 1) + np.eye(n)
    return np.asfortranarray(Q), d, np.asfortranarray(R)
def factors(n, seed=7):
    rng = np.random.default_rng(seed + n)
    return factor(rng, n), factor(rng, n)
out = {}
for n in %(sizes)r:
    F1, F2 = factors(n)
    out["G2_%%d" %% n] = hip.inv_I_plus_ldr_mul_ldr(F1, F2)
    G, ld = hip.inv_I_plus_ldr(F1)
    out["G1_%%d" %% n] = G; out["ld_%%d" %% n] = np.float64(ld)
# state between calls (rowpos parity, log det accumulation, the flag): A, B, A through the same workspace
for n in %(seq_sizes)r:
    A = factors(n); B = factors(n, seed=1007)
    for i, (F1, F2) in enumerate((A, B, A)):
        out["seq%%d_G2_%%d" %% (i, n)] = hip.inv_I_plus_ldr_mul_ldr(F1, F2)
        G, ld = hip.inv_I_plus_ldr(F1)
        out["seq%%d_G1_%%d" %% (i, n)] = G; out["seq%%d_ld_%%d" %% (i, n)] = np.float64(ld)
# the chain dimension: three chains in one engine at N = 96 (<4,1> with two live waves), one forward and one backward sweep
if %(chains)d:
    m = dqmc_amd.HubbardModel(L1=12, L2=8, U=4.0, beta=1.0, nt=10, n_stab=5); C = %(chains)d
    f = np.stack([m.random_fields(60 + c) for c in range(C)])
    e = m.engine(hip, n_chains=C); e.set_fields(f); e.init()
    rng = np.random.default_rng(18)
    for sweep in ("sweep_0_to_beta", "sweep_beta_to_0"):
        streams = [m.random_stream(rng) for _ in range(C)]
        getattr(e, sweep)(*(np.stack([st[k] for st in streams]) for k in range(3)))
        out["chains_G_" + sweep] = e.get_G(); out["chains_fields_" + sweep] = e.get_fields()
    del e
# singular pivot, last: M = R^-1 diag(1 / max(d, 1)) + L diag(min(d, 1)) with R = I, L = -I is diag(1/2 - 1) except for an exactly
# zero row and column where d = 1 (column 70: the tail panel).  A status, no fault; the call after it is clean again.
n = 72
d = np.full(n, 2.0); d[70] = 1.0
try:
    hip.inv_I_plus_ldr((np.asfortranarray(-np.eye(n)), d, np.asfortranarray(np.eye(n))))
    out["singular_code"] = np.int64(0)
except DqmcError as err:
    out["singular_code"] = np.int64(err.code)
F1, F2 = factors(n)
out["after_singular_G2"] = hip.inv_I_plus_ldr_mul_ldr(F1, F2)
np.savez(sys.argv[1], **out)
print("ok")
"""


def _run_form(path, two_launch):
    env = dict(os.environ)
    env.pop("DQMC_LU_CLASSIC", None)
    env["DQMC_GJ_FUSED"] = "0" if two_launch else "1"
    code = WORKER % dict(root=ROOT, sizes=SIZES, seq_sizes=SEQ_SIZES, chains=CHAINS)
    out = subprocess.run([sys.executable, "-c", code, path], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-2000:]
    return dict(np.load(path))


@pytest.fixture(scope="module")
def forms(tmp_path_factory):
    """{name: array} of the fused form and of the two-launch form: one subprocess each, shared by every case below and never modified"""
    d = tmp_path_factory.mktemp("fused_gj")
    return _run_form(str(d / "fused.npz"), False), _run_form(str(d / "two_launch.npz"), True)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same_bits(a, b):
    return bool((_bits(a) == _bits(b)).all())


@pytest.mark.parametrize("n", SIZES)
def test_gj_fused_step_bitwise_equals_two_launch_form(forms, n):
    """G of inv_I_plus_ldr_mul_ldr (no log det) and (G, log det) of inv_I_plus_ldr (accumulated log det): the same bits in both forms"""
    fused, two = forms
    for name in ("G2_%d" % n, "G1_%d" % n, "ld_%d" % n):
        a, b = fused[name], two[name]
        assert np.isfinite(a).all(), name
        assert _same_bits(a, b), "%s differs: max|diff| = %.3e" % (name, np.abs(a - b).max())


@pytest.mark.parametrize("n", SEQ_SIZES)
def test_gj_fused_step_keeps_no_state_between_calls(forms, n):
    """solve(A), solve(B), solve(A) in one process: the first and the third result are the same bits, and B's are B's own in both forms"""
    fused, two = forms
    for part in ("G2", "G1", "ld"):
        assert _same_bits(fused["seq0_%s_%d" % (part, n)], fused["seq2_%s_%d" % (part, n)]), part
        assert _same_bits(fused["seq0_%s_%d" % (part, n)], fused["%s_%d" % (part, n)]), part
        assert _same_bits(fused["seq1_%s_%d" % (part, n)], two["seq1_%s_%d" % (part, n)]), part
        assert not _same_bits(fused["seq1_%s_%d" % (part, n)], fused["seq0_%s_%d" % (part, n)]), part
        assert np.isfinite(fused["seq1_%s_%d" % (part, n)]).all(), part


def test_three_chains_on_the_fused_gj_step(forms, orc):
    """Three chains in one engine at N = 96 (12 x 8, nt = 10, n_stab = 5) with DQMC_GJ_FUSED=1: the chain dimension of rowpos, log det and
    the tiles.  One forward and one backward sweep, per chain against the oracle: fields identical, max|dG| <= 1e-10 max(1, max|G|)."""
    from dqmc_amd import HubbardModel
    fused, two = forms
    m = HubbardModel(L1=12, L2=8, U=4.0, beta=1.0, nt=10, n_stab=5); C = CHAINS
    f = np.stack([m.random_fields(60 + c) for c in range(C)])
    os_ = []
    for c in range(C):
        o = m.engine(orc); o.set_fields(f[c]); o.init(); os_.append(o)
    rng = np.random.default_rng(18)
    for sweep in ("sweep_0_to_beta", "sweep_beta_to_0"):
        streams = [m.random_stream(rng) for _ in range(C)]
        G = fused["chains_G_" + sweep]; fe = fused["chains_fields_" + sweep]
        assert _same_bits(G, two["chains_G_" + sweep]), sweep
        for c in range(C):
            getattr(os_[c], sweep)(*streams[c])
            Go = os_[c].get_G()
            assert (fe[c] == os_[c].get_fields()).all(), (sweep, c)
            err = np.abs(G[c] - Go).max()
            print(f"{sweep} chain {c}: max|dG| = {err:.3e}, max|G| = {np.abs(Go).max():.3e}")
            assert err <= 1e-10 * max(1.0, np.abs(Go).max()), (sweep, c)


def test_singular_pivot_raises_the_same_status_in_both_forms(forms):
    """an exactly zero column at n = 72 (in the tail panel): DQMC_ENUMERIC in both forms, no fault, and the next solve is clean"""
    fused, two = forms
    assert int(fused["singular_code"]) != 0
    assert int(fused["singular_code"]) == int(two["singular_code"])
    assert _same_bits(fused["after_singular_G2"], fused["G2_72"])
    assert _same_bits(two["after_singular_G2"], two["G2_72"])
