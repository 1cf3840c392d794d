"""The one-launch-per-panel form of the panel-pivoted to_LDR (qp_step_kernel, qr_panel.hip) against the two-launch form it replaces
(qp_panel_kernel + qp_update_kernel, kept behind DQMC_QR_PANEL_FUSED=0; =1 takes the fused step wherever it has an instance).

Every workgroup of the fused step factors the panel with the device function the panel kernel uses, and its update keeps the operand
partition of the MFMAs and the order of the cross-wave sums, so L, d and R are expected BITWISE equal, not close.  The switches are read
once per process: each form computes all cases in one subprocess of its own and leaves them in a file.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from dqmc_amd import HubbardModel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# 64: single-wave instance, 4 panels (first and last step only differ in the grid); 80: second wave mostly empty, odd tile count;
# 144, 256: <4,1>; 272: <4,2>, 17 tiles; 576: <3,3>; 592: above the fused step's largest instance -- the two-launch form in both processes
SIZES = (64, 80, 144, 256, 272, 576, 592)
KINDS = ("graded", "both")

WORKER = r"""
import sys, numpy as np
sys.path.insert(0, %(root)r)
import dqmc_amd
hip = dqmc_amd.lib()
def matrix(n, kind):
    if kind == "graded":       # tests/test_gpu_parity.py::graded
        rng = np.random.default_rng(100 + n)
        return rng.standard_normal((n, n)) * np.exp(rng.uniform(-6, 6, n))[None, :]
    rng = np.random.default_rng(900 + n)       # ... ::test_to_ldr_panel_on_strongly_graded_matrices, kind "both"
    X = rng.standard_normal((n, n)); s1 = np.exp(rng.uniform(-28, 28, n)); s2 = np.exp(rng.uniform(-28, 28, n))
    return s1[:, None] * X * s2[None, :]
out = {}
for n in %(sizes)r:
    for kind in %(kinds)r:
        L, d, R = hip.to_ldr(matrix(n, kind))
        out["L_%%d_%%s" %% (n, kind)] = L; out["d_%%d_%%s" %% (n, kind)] = d; out["R_%%d_%%s" %% (n, kind)] = R
# state between calls (ticket counter, sketch parity, pivpos): A, B, A through the same workspace
for n in (64, 80):
    A = matrix(n, "graded"); B = matrix(n, "both")
    for i, M in enumerate((A, B, A)):
        L, d, R = hip.to_ldr(M)
        out["seq%%d_L_%%d" %% (i, n)] = L; out["seq%%d_d_%%d" %% (i, n)] = d; out["seq%%d_R_%%d" %% (i, n)] = R
np.savez(sys.argv[1], **out)
print("ok")
"""


def _run_form(path, two_launch):
    env = dict(os.environ)
    env.pop("DQMC_QR_PANEL", None)
    env["DQMC_QR_PANEL_FUSED"] = "0" if two_launch else "1"
    code = WORKER % dict(root=ROOT, sizes=SIZES, kinds=KINDS)
    out = subprocess.run([sys.executable, "-c", code, path], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-2000:]
    return dict(np.load(path))


@pytest.fixture(scope="module")
def forms(tmp_path_factory):
    """{name: array} of the fused form and of the two-launch form: one subprocess each, shared by every case below and never modified"""
    d = tmp_path_factory.mktemp("fused_panels")
    return _run_form(str(d / "fused.npz"), False), _run_form(str(d / "two_launch.npz"), True)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_to_ldr_fused_step_bitwise_equals_two_launch_form(forms, n, kind):
    fused, two = forms
    for part in "LdR":
        a, b = fused["%s_%d_%s" % (part, n, kind)], two["%s_%d_%s" % (part, n, kind)]
        assert np.isfinite(a).all()
        assert (_bits(a) == _bits(b)).all(), "%s differs at n = %d (%s): max|diff| = %.3e" % (part, n, kind, np.abs(a - b).max())


@pytest.mark.parametrize("n", [64, 80])
def test_to_ldr_fused_step_keeps_no_state_between_calls(forms, n):
    """to_ldr(A), to_ldr(B), to_ldr(A) in one process: the first and the third result are the same bits, and B's are B's own"""
    fused, two = forms
    for part in "LdR":
        assert (_bits(fused["seq0_%s_%d" % (part, n)]) == _bits(fused["seq2_%s_%d" % (part, n)])).all(), part
        assert (_bits(fused["seq0_%s_%d" % (part, n)]) == _bits(fused["%s_%d_graded" % (part, n)])).all(), part
        assert (_bits(fused["seq1_%s_%d" % (part, n)]) == _bits(fused["%s_%d_both" % (part, n)])).all(), part
        assert (_bits(fused["seq1_%s_%d" % (part, n)]) == _bits(two["seq1_%s_%d" % (part, n)])).all(), part


def test_three_chains_on_the_panel_path(hip, orc):
    """Three chains in one engine at N = 64 (the smallest size on the panel path): the chain dimension of the sketch buffers and ticket
    counters.  One forward and one backward sweep, per chain against the oracle: fields identical, max|dG| <= 1e-10 max(1, max|G|)."""
    m = HubbardModel(L1=8, L2=8, U=4.0, beta=1.0, nt=10, n_stab=5); C = 3
    f = np.stack([m.random_fields(60 + c) for c in range(C)])
    e = m.engine(hip, n_chains=C); e.set_fields(f); e.init()
    os_ = []
    for c in range(C):
        o = m.engine(orc); o.set_fields(f[c]); o.init(); os_.append(o)
    rng = np.random.default_rng(18)
    for sweep in ("sweep_0_to_beta", "sweep_beta_to_0"):
        streams = [m.random_stream(rng) for _ in range(C)]
        getattr(e, sweep)(*(np.stack([st[k] for st in streams]) for k in range(3)))
        G = e.get_G(); fe = e.get_fields()
        for c in range(C):
            getattr(os_[c], sweep)(*streams[c])
            Go = os_[c].get_G()
            assert (fe[c] == os_[c].get_fields()).all(), (sweep, c)
            err = np.abs(G[c] - Go).max()
            print(f"{sweep} chain {c}: max|dG| = {err:.3e}, max|G| = {np.abs(Go).max():.3e}")
            assert err <= 1e-10 * max(1.0, np.abs(Go).max()), (sweep, c)
