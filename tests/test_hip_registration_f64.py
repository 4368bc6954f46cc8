"""kabsch_kernel (csrc/match.hip with the fp64 Jacobi of csrc/svd3.h, through ops.kabsch, ops.kabsch_codes, ops.kabsch_residual_matrix and its
batch form) and icp_kernel (csrc/icp.hip, through ops.icp with LS_FLAG_CONTRACT_FMA off and on) against the float64 oracles of
tests/registration_oracle.py at their size edges.  The cases, their inputs and the rule are tests/tools/registration_vs_float64.py:
per PROBLEM and per measure, relative to the problem's scale s = max(1, largest |coordinate|),
    err <= min(16 x e32, 1e-4),
e32 the same measure of the float32 oracle, computed here on the CPU from the same inputs; the preconditions on the inputs (gap >= 0.01,
e32_min <= e32 <= 1e-5; for ICP the certificate that pins the trajectory, so that iteration counts and final assignments are compared exactly)
are asserted with every comparison and are what tests/test_registration_oracle_cpu.py checks without a GPU.  Every test prints the largest
err / e32 per entry, path and measure."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TOOL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools", "registration_vs_float64.py")


def _load():
    spec = importlib.util.spec_from_file_location("registration_vs_float64", TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


lad = _load()   # one module object: the references it caches serve every test of this file
F64 = np.float64


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _done(what, table, bad):
    print(f"[{what}] largest err / e32 per entry, path and measure\n{lad.format_table(table)}")
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad[:20])


# ------------------------------------------------------------------------------------------------ Kabsch
@pytest.mark.parametrize("n", lad.KB_N)
def test_kabsch_vs_float64_per_problem(n):
    """ops.kabsch at one point count: b = 1, 3, 4, 5 problems x generic / planar / reflected / far clouds x no / random / raw thresholded
    weights.  Status 0 everywhere; R, t / s and res / s of every problem under the rule."""
    table, bad = {}, []
    lad.check_kabsch([c for c in lad.kabsch_ladder() if c[1] == n], _dev(), table, bad)
    _done(f"kabsch n={n}", table, bad)


def test_kabsch_codes_vs_float64_per_problem():
    """ops.kabsch_codes: pseudo-points fl32(z + t) of width 70, 256, 257, 300; no selector, sel2 alone, both; negative and repeated entries"""
    table, bad = {}, []
    lad.check_codes(lad.codes_ladder(), _dev(), table, bad)
    _done("kabsch_codes", table, bad)


def test_kabsch_residual_matrix_vs_float64_per_problem():
    """ops.kabsch_residual_matrix at (n, m, P) = (1, 1, 70), (3, 5, 257), (5, 3, 300), (7, 6, 256) and, per width, a ragged batch of four
    matrices with an empty problem between them through ops.kabsch_residual_matrix_batch (which must also return the single calls' bits):
    mean_res / s of every matrix under the rule, every entry on its own scale"""
    table, bad = {}, []
    lad.check_resmat(lad.resmat_ladder(), _dev(), table, bad)
    _done("kabsch_residual_matrix", table, bad)


def test_rank_deficient_kabsch_by_property():
    """One and two points: the least-squares rotation is a family, so nothing is compared with the oracle.  The status is the rank of the
    covariance AS THE KERNEL FORMS IT, in float32 (svd3.h: a singular value counts as zero below 1e-150).  That rank is exact only where the
    arithmetic is: x1 at the origin gives H = 0 and RANK0 with the identity; x1 on a line through the origin whose direction has
    power-of-two ratios, (1, 2, -4), makes the rows of H exact multiples of one another and gives RANK1 (a single such point: RANK1, or
    RANK0 should its mean reproduce it).  A generic pair has a covariance of rank 2 by rounding, 1e-8 of its size, and reports status 0
    with one member of the family (measured: 0 for five pairs of five, 1 for five single points of five); for generic inputs no status is
    asserted.  Whatever the status, R is a proper rotation and t = mu2 - R mu1 to float32 rounding at the scale of the data."""
    from livingscenes_amd import _lib, ops
    dev = _dev()
    rng = np.random.default_rng(11)
    line = np.array([1.0, 2.0, -4.0])
    x2_1, x2_2 = rng.standard_normal((5, 1, 3)) + 2.0, rng.standard_normal((5, 2, 3)) + 2.0
    cases = {
        "n=1 origin": (np.zeros((5, 1, 3)), x2_1, {_lib.KABSCH_RANK0}),
        "n=1 exact": (rng.uniform(0.5, 1.5, (5, 1, 1)) * line, x2_1, {_lib.KABSCH_RANK1, _lib.KABSCH_RANK0}),
        "n=2 exact": (rng.uniform(-1.5, 1.5, (5, 2, 1)) * line, x2_2, {_lib.KABSCH_RANK1}),
        "n=1 generic": (rng.standard_normal((5, 1, 3)), x2_1, {_lib.KABSCH_OK, _lib.KABSCH_RANK1, _lib.KABSCH_RANK0}),
        "n=2 generic": (rng.standard_normal((5, 2, 3)), x2_2, {_lib.KABSCH_OK, _lib.KABSCH_RANK1, _lib.KABSCH_RANK0}),
    }
    for name, (x1, x2, allowed) in cases.items():
        x1, x2 = x1.astype(np.float32), x2.astype(np.float32)
        R, t, res, fl = (o.cpu().numpy() for o in ops.kabsch(torch.from_numpy(x1).to(dev), torch.from_numpy(x2).to(dev), return_flags=True))
        print(f"{name}: status {fl.tolist()}")
        assert set(fl.tolist()) <= allowed, (name, fl.tolist())
        for p in range(5):
            Rp = R[p].astype(F64)
            s = lad.scale_of(x1[p], x2[p])
            assert np.abs(Rp.T @ Rp - np.eye(3)).max() < 8 * 2.0 ** -24 and np.linalg.det(Rp) > 0.999, (name, p)
            if _lib.KABSCH_RANK0 in allowed and len(allowed) == 1:
                assert np.array_equal(R[p], np.eye(3, dtype=np.float32)), (name, p)
            # the means carry (1 + eps) factors of 1e-7; three products and three sums of values up to s
            assert np.abs(t[p].reshape(3) - (x2[p].astype(F64).mean(0) - Rp @ x1[p].astype(F64).mean(0))).max() <= 16 * 2.0 ** -24 * s, (name, p)


# ------------------------------------------------------------------------------------------------ ICP
ICP_CASES = lad.icp_ladder()


@pytest.mark.parametrize("case", ICP_CASES, ids=[c[0] for c in ICP_CASES])
def test_icp_vs_float64(case):
    """One problem, LS_FLAG_CONTRACT_FMA off and on: the oracle's iteration count; the oracle's final assignment, recomputed on the CPU in
    float64 from the kernel's pose; R, T / s and rmse / s under the rule."""
    table, bad = {}, []
    lad.check_icp([case], _dev(), table, bad)
    _done(case[0], table, bad)


def test_icp_batch_equals_its_single_calls_bit_for_bit():
    """three certified problems of one shape that stop after 3, 4 and 5 iterations: every problem of the batch stops on its own criterion"""
    from livingscenes_amd import _lib, ops
    dev = _dev()
    X, Y, R0, T0, its = lad.icp_batch_inputs()
    X, Y, R0, T0 = (torch.from_numpy(a).to(dev) for a in (X, Y, R0, T0))
    for flags in (0, _lib.FLAG_CONTRACT_FMA):
        batch = ops.icp(X, Y, R0, T0, flags=flags)
        assert batch[3].tolist() == its, (batch[3].tolist(), its)
        for p in range(3):
            one = ops.icp(X[p:p + 1], Y[p:p + 1], R0[p:p + 1], T0[p:p + 1], flags=flags)
            assert all(torch.equal(a[p:p + 1], b) for a, b in zip(batch, one)), (flags, p)


@pytest.mark.parametrize("n,m,msg", [(lad.ICP_N_MAX + 1, 8, "icp: source cloud too large (n=4097, max 4096)"),
                                     (8, lad.ICP_M_MAX + 1, "icp: target cloud too large for LDS (m=10241, max 10240)")])
def test_icp_refuses_a_cloud_beyond_its_limits_and_writes_nothing(n, m, msg):
    from livingscenes_amd import _lib, ops
    dev = _dev()
    g = torch.Generator().manual_seed(n + m)
    X, Y = torch.rand(2, n, 3, generator=g).to(dev), torch.rand(2, m, 3, generator=g).to(dev)
    R0, T0 = torch.eye(3).repeat(2, 1, 1).to(dev), torch.zeros(2, 3, device=dev)
    outs = [torch.full(s, 7.0, dtype=torch.float32, device=dev) for s in ((2, 3, 3), (2, 3), (2,))] + [torch.full((2,), 7, dtype=torch.int32, device=dev)]
    lib = _lib.load()
    ws = torch.full((max(int(lib.ls_icp_workspace_bytes(2, n)), 1),), 0x5A, dtype=torch.uint8, device=dev)
    for flags in (0, _lib.FLAG_CONTRACT_FMA):
        with torch.cuda.device(dev):
            rc = lib.ls_icp_f32(ops.ptr(X), ops.ptr(Y), ops.ptr(R0), ops.ptr(T0), 2, n, m, 100, 1e-6, flags, *[ops.ptr(o) for o in outs], ops.ptr(ws),
                                ws.numel(), ops.stream_ptr(dev))
        got = lib.ls_last_error().decode()
        torch.cuda.synchronize()
        assert rc == -1 and got == msg, (rc, got)                                  # LS_ERR_INVALID
        assert all(bool((o == 7).all()) for o in outs) and bool((ws == 0x5A).all())
    with pytest.raises(_lib.LsError, match="too large"):
        ops.icp(X, Y, R0, T0)
