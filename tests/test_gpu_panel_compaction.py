"""Late pivot panels on one wave (qr_panel.hip: select_step_cw, lu_gj.hip: gj_step_cw) against the chains that keep every column / row on
its original lane to the last panel (DQMC_PANEL_COMPACT=0), in the fused and in the two-launch form of both.

The compacted chains do the same arithmetic on the same numbers, and their pivot rules are functions of the values alone (QR: a maximum
over distinct keys that carry the original column; Gauss-Jordan: the lowest row among those with the largest |a| truncated to 43 mantissa
bits, inside a wave as between waves), so every result is expected BITWISE equal across the three switch states, exact ties included.
The switches are read once per process: each state computes all cases in one subprocess of its own and leaves them in a file.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# to_LDR: 144 three waves, five uncompacted panels (144 .. 80 live columns), then four on one wave (64 .. 16); 192, 256: the flagship
# instance; 128 and 272: the <2,1> and <4,2> instances, which the change must leave alone
QR_SIZES = (128, 144, 192, 256, 272)
# solve: 136 tail panel of 8 columns with 8 live rows; 200: 200, 168, 136 live rows uncompacted, then 104, 72 (two per lane), 40, 8
GJ_SIZES = (136, 200, 256)
STATES = ("default", "uncompacted", "two_launch")
ENV = {"default": {}, "uncompacted": {"DQMC_PANEL_COMPACT": "0"}, "two_launch": {"DQMC_QR_PANEL_FUSED": "0", "DQMC_GJ_FUSED": "0"}}

WORKER = r"""
import sys, numpy as np
sys.path.insert(0, %(root)r)
import dqmc_amd
from dqmc_amd import fixtures
from dqmc_amd.abi import DqmcError
hip = dqmc_amd.lib()
def factor(rng, n):            # tests/test_gpu_fused_gj.py: orthogonal L, d graded over e^+-8, unit upper R
    Q = np.linalg.qr(rng.standard_normal((n, n)))[0]
    d = np.exp(np.sort(rng.uniform(-8, 8, n))[::-1])
    R = np.triu(rng.standard_normal((n, n)) * 0.2, 1) + np.eye(n)
    return np.asfortranarray(Q), d, np.asfortranarray(R)
def factors(n, seed=7):
    rng = np.random.default_rng(seed + n)
    return factor(rng, n), factor(rng, n)
def product(n):
    Q, d, R = factors(n)[0]
    return (Q * d[None, :]) @ R
def hadamard(n):
    H = np.ones((1, 1))
    while H.shape[0] < n:
        H = np.block([[H, H], [H, -H]])
    return H
out = {}
for n in %(qr_sizes)r:
    L, d, R = hip.to_ldr(product(n))
    out["L_%%d" %% n] = L; out["d_%%d" %% n] = d; out["R_%%d" %% n] = R
# exact norm ties between columns that start in different waves (3, 77 | 200) and meet in one
M = product(256); M[:, 200] = M[:, 3]; M[:, 77] = M[:, 3]
L, d, R = hip.to_ldr(M)
out["tie_M"] = M; out["tie_L"] = L; out["tie_d"] = d; out["tie_R"] = R
for n in %(gj_sizes)r:
    F1, F2 = factors(n)
    out["G2_%%d" %% n] = hip.inv_I_plus_ldr_mul_ldr(F1, F2)
    G, ld = hip.inv_I_plus_ldr(F1)
    out["G1_%%d" %% n] = G; out["ld_%%d" %% n] = np.float64(ld)
# state between calls: A, B, A through the same workspace
n = 136
A = factors(n); B = factors(n, seed=1007)
for i, (F1, F2) in enumerate((A, B, A)):
    out["seq%%d_G2" %% i] = hip.inv_I_plus_ldr_mul_ldr(F1, F2)
    G, ld = hip.inv_I_plus_ldr(F1)
    out["seq%%d_G1" %% i] = G; out["seq%%d_ld" %% i] = np.float64(ld)
# ties: M = I/2 + H/16 (H the 256 Sylvester Hadamard matrix, H/16 orthogonal): partial pivoting meets exact ties and 43-bit near-ties
n = 256
G, ld = hip.inv_I_plus_ldr((np.asfortranarray(hadamard(n) / 16.0), np.full(n, 2.0), np.asfortranarray(np.eye(n))))
out["had_G"] = G; out["had_ld"] = np.float64(ld)
# sweeps: 16 x 12 sites (N = 192), one chain, one forward and one backward sweep
m = dqmc_amd.HubbardModel(L1=16, L2=12, U=4.0, beta=1.0, nt=10, n_stab=5)
e = m.engine(hip); e.set_fields(m.random_fields(61)); e.init()
rng = np.random.default_rng(19)
for sweep in ("sweep_0_to_beta", "sweep_beta_to_0"):
    getattr(e, sweep)(*m.random_stream(rng))
    out["sw_G_" + sweep] = e.get_G(); out["sw_fields_" + sweep] = e.get_fields()
del e
# the thermalised cfg-3 fixture: init plus one sweep
if %(cfg3)d:
    z, m3, st = fixtures.load("cfg3_therm")
    e = m3.engine(hip); e.set_fields(z["fields"]); e.init()
    out["cfg3_G_init"] = e.get_G()
    e.sweep_0_to_beta(*st[0]); e.sweep_beta_to_0(*st[1])
    out["cfg3_G"] = e.get_G(); out["cfg3_fields"] = e.get_fields()
    del e
# singular pivot in a compacted panel, last: M = diag(1/2 - 1) except for an exactly zero row and column 130 (the tail panel of n = 136,
# whose 8 live rows stand in wave 2).  A status, no fault; the call after it is clean again.
n = 136
d = np.full(n, 2.0); d[130] = 1.0
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


def _run_state(path, state):
    env = dict(os.environ)
    for k in ("DQMC_LU_CLASSIC", "DQMC_QR_PANEL", "DQMC_PANEL_COMPACT", "DQMC_QR_PANEL_FUSED", "DQMC_GJ_FUSED"):
        env.pop(k, None)
    env.update(ENV[state])
    code = WORKER % dict(root=ROOT, qr_sizes=QR_SIZES, gj_sizes=GJ_SIZES, cfg3=0 if state == "two_launch" else 1)
    out = subprocess.run([sys.executable, "-c", code, path], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-2000:]
    return dict(np.load(path))


@pytest.fixture(scope="module")
def states(tmp_path_factory):
    """{state: {name: array}}: one subprocess per switch state, shared by every case below and never modified"""
    d = tmp_path_factory.mktemp("panel_compaction")
    return {s: _run_state(str(d / (s + ".npz")), s) for s in STATES}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same_bits(a, b):
    return a.shape == b.shape and bool((_bits(a) == _bits(b)).all())


def _all_same(states, name):
    ref = states["default"][name]
    assert np.isfinite(ref).all(), name
    for s in STATES[1:]:
        assert _same_bits(ref, states[s][name]), "%s differs in state %s: max|diff| = %.3e" % (name, s, np.abs(ref - states[s][name]).max())


@pytest.mark.parametrize("n", QR_SIZES)
def test_to_ldr_bitwise_equal_in_all_switch_states(states, n):
    for part in "LdR":
        _all_same(states, "%s_%d" % (part, n))


def test_to_ldr_exact_norm_ties_across_waves(states):
    """columns 3, 77 and 200 of a 256 matrix are equal: the lowest column wins wherever the three stand; L diag(d) R is the matrix"""
    for part in "LdR":
        _all_same(states, "tie_" + part)
    z = states["default"]
    M = z["tie_M"]
    err = np.abs((z["tie_L"] * z["tie_d"][None, :]) @ z["tie_R"] - M).max() / np.abs(M).max()
    print(f"tie-break: max|L d R - M| / max|M| = {err:.3e}")
    assert err <= 1e-12


@pytest.mark.parametrize("n", GJ_SIZES)
def test_solve_bitwise_equal_in_all_switch_states(states, n):
    for name in ("G2_%d" % n, "G1_%d" % n, "ld_%d" % n):
        _all_same(states, name)


def test_solve_keeps_no_state_between_calls(states):
    """solve(A), solve(B), solve(A) at n = 136: the first and the third result are the same bits, and B's are B's own"""
    for s in STATES:
        z = states[s]
        for part in ("G2", "G1", "ld"):
            assert _same_bits(z["seq0_" + part], z["seq2_" + part]), (s, part)
            assert _same_bits(z["seq0_" + part], z["%s_136" % part]), (s, part)
            assert not _same_bits(z["seq1_" + part], z["seq0_" + part]), (s, part)
    for part in ("G2", "G1", "ld"):
        _all_same(states, "seq1_" + part)


def test_solve_with_exact_pivot_ties(states):
    """M = I/2 + H/16, cond 3: G = (I + H/8)^-1 against numpy.linalg.solve at the project's parity bar, the same bits in every state"""
    _all_same(states, "had_G"); _all_same(states, "had_ld")
    n = 256
    H = np.ones((1, 1))
    while H.shape[0] < n:
        H = np.block([[H, H], [H, -H]])
    ref = np.linalg.solve(np.eye(n) + H / 8.0, np.eye(n))
    G = states["default"]["had_G"]
    err = np.abs(G - ref).max()
    print(f"Hadamard ties: max|dG| = {err:.3e}, max|G| = {np.abs(ref).max():.3e}")
    assert err <= 1e-10 * max(1.0, np.abs(ref).max())


def test_singular_pivot_in_a_compacted_panel(states):
    """an exactly zero row and column 130 at n = 136: the same non-zero status in every state, no fault, and the next solve is clean"""
    code = int(states["default"]["singular_code"])
    assert code != 0
    for s in STATES:
        assert int(states[s]["singular_code"]) == code, s
        assert _same_bits(states[s]["after_singular_G2"], states[s]["G2_136"]), s


def test_sweeps_at_192_sites(states, orc):
    """16 x 12 sites, nt = 10, n_stab = 5, one chain: fields identical to the oracle's, max|dG| <= 1e-10 max(1, max|G|), G bitwise equal
    between the switch states"""
    from dqmc_amd import HubbardModel
    m = HubbardModel(L1=16, L2=12, U=4.0, beta=1.0, nt=10, n_stab=5)
    o = m.engine(orc); o.set_fields(m.random_fields(61)); o.init()
    rng = np.random.default_rng(19)
    for sweep in ("sweep_0_to_beta", "sweep_beta_to_0"):
        getattr(o, sweep)(*m.random_stream(rng))
        _all_same(states, "sw_G_" + sweep)
        G = states["default"]["sw_G_" + sweep]; Go = o.get_G()
        for s in STATES:
            assert (states[s]["sw_fields_" + sweep] == o.get_fields()).all(), (sweep, s)
        err = np.abs(G - Go).max()
        print(f"{sweep}: max|dG| = {err:.3e}, max|G| = {np.abs(Go).max():.3e}")
        assert err <= 1e-10 * max(1.0, np.abs(Go).max()), sweep


def test_cfg3_thermalised_sweep_on_and_off(states):
    """the thermalised cfg-3 fixture, init plus one sweep: fields and G bitwise equal with and without the compaction"""
    on, off = states["default"], states["uncompacted"]
    assert np.isfinite(on["cfg3_G"]).all()
    assert _same_bits(on["cfg3_G_init"], off["cfg3_G_init"])
    assert (on["cfg3_fields"] == off["cfg3_fields"]).all()
    assert _same_bits(on["cfg3_G"], off["cfg3_G"]), "max|diff| = %.3e" % np.abs(on["cfg3_G"] - off["cfg3_G"]).max()
