"""The GP stage at its edges: roma_cos_kernel, roma_chol_diag_block, roma_chol_step, roma_chol_subst_step, ops.spd_solve and
GP.posterior_rows against the plain fp64 references of tests/gp_ref.py (written from the contracts in include/roma_hip.h).
Run with -m gpu on an MI355X.

Tolerances.  The GEMM-like parts of the solver kernels (R, the trailing update, X, T) are held to the elementwise fp32 product bound
of gp_ref.product_bound / step_bounds, the 64 x 64 factorisations to the perturbation bound of gp_ref.factor_bounds; the inputs of
every such case are fp32 numbers prepared in fp64 on the host, so a case depends on no kernel that ran before it.  spd_solve and
cos_kernel keep the bounds their existing tests in test_gpu_ops.py use; the ill-conditioned solves are measured against LAPACK's fp32
Cholesky solve of the same system."""
import pytest
import torch

from tests import gp_ref as G
from tests import helpers as H

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"
NB = G.NB
SENT = -777.25                                                     # sentinel of every padded buffer (exact in fp32)


def _ops():
    from roma_amd import ops
    return ops


def _abi():
    from roma_amd import _lib
    return _lib.load(), _lib.check


def _st():
    return torch.cuda.current_stream().cuda_stream


def _padded(t, rows, ld):
    """(B, r, c) -> device fp32 buffer (B, rows, ld) filled with the sentinel, t in its top-left corner."""
    B, r, c = t.shape
    buf = torch.full((B, rows, ld), SENT, dtype=torch.float32)
    buf[:, :r, :c] = t.float()
    return buf.to(DEV)


def _within(got, ref, bound, what):
    """got (fp32 values) within the elementwise bound of ref; prints the worst ratio before asserting."""
    err = (got.double() - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f"{what}: max err {float(err.max()) if err.numel() else 0.0:.2e}, worst err/bound {ratio:.3f}")
    assert bool((err <= bound).all()), what


# ---- 2. roma_chol_diag_block ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [1, 15, 16, 17, 33, 63, 64])
def test_diag_block_against_fp64(nb):
    lib, check = _abi()
    B, lda, ldw, rows = 3, nb + 5, nb + 3, nb + 2
    K, _ = G.well_conditioned_system(B, nb, 1, seed=100 + nb)
    blk = torch.tril(K) + torch.triu(torch.full_like(K, 1e6), 1)     # only the lower triangle is read: the upper one holds a marker
    A = _padded(blk, rows, lda)
    A0 = A.clone()
    W = torch.full((B, rows, ldw), SENT, dtype=torch.float32, device=DEV)
    info = torch.zeros(B, dtype=torch.int32, device=DEV)
    check(lib.roma_chol_diag_block(A.data_ptr(), lda, A.stride(0), W.data_ptr(), ldw, W.stride(0), nb, B, info.data_ptr(), 0, _st()), "diag")
    torch.cuda.synchronize()
    A, A0, W = A.cpu(), A0.cpu(), W.cpu()
    L, Wi, tolL, tolW = G.factor_bounds(K.double())
    eL = (torch.tril(A[:, :nb, :nb]).double() - L).abs().amax(dim=(1, 2))
    eW = (W[:, :nb, :nb].double() - Wi).abs().amax(dim=(1, 2))
    print(f"nb={nb}: |L - ref| {eL.tolist()} (bound {tolL.tolist()}), |W - ref| {eW.tolist()} (bound {tolW.tolist()})")
    assert bool((eL <= tolL).all()) and bool((eW <= tolW).all())
    assert torch.equal(torch.triu(A[:, :nb, :nb], 1), torch.triu(A0[:, :nb, :nb], 1))        # strict upper triangle of the block
    outside = torch.ones_like(A, dtype=torch.bool)
    outside[:, :nb, :nb] = False
    assert torch.equal(A[outside], A0[outside])                                              # nothing outside the block
    assert float(torch.triu(W[:, :nb, :nb], 1).abs().max() if nb > 1 else 0.0) == 0.0       # W exactly zero above its diagonal
    outside = torch.ones_like(W, dtype=torch.bool)
    outside[:, :nb, :nb] = False
    assert bool((W[outside] == SENT).all())
    assert int(info.abs().max()) == 0


# ---- 3. roma_chol_step ------------------------------------------------------------------------------------------------------------
STEP_CASES = {
    # name: (n, m, j, nb, lda - ncols, ldr - ncols, ldw = ldwn)
    "middle": (200, 24, 64, 64, 0, 0, 64),
    "next_narrow": (200, 24, 128, 64, 0, 0, 64),
    "next_narrow_m_straddles": (130, 70, 64, 64, 0, 0, 64),
    "own_narrow_last": (200, 24, 192, 8, 0, 0, 64),
    "exact_multiple_first": (128, 5, 0, 64, 0, 0, 64),
    "exact_multiple_last": (128, 5, 64, 64, 0, 0, 64),
    "single_block": (40, 3, 0, 40, 0, 0, 64),
    "wide_pitch": (200, 24, 64, 64, 7, 3, 72),
}


@pytest.mark.parametrize("name", list(STEP_CASES))
def test_chol_step_against_its_definition(name):
    lib, check = _abi()
    n, m, j, nb, pa, pr, ldw = STEP_CASES[name]
    B, ncols, e = 2, n + m, j + nb
    lda, ldr = ncols + pa, ncols + pr
    K, F = G.well_conditioned_system(B, n, m, seed=1000 + n + j)
    A32 = G.state_before_step(K, F, j).float()                        # the matrix as it stands when this step begins, fp32-stored
    W32 = torch.linalg.inv(torch.linalg.cholesky(A32[:, j:e, j:e].double())).float()
    last = e == n
    A = _padded(A32, n + 1, lda)
    A0 = A.cpu()
    W = _padded(W32, NB, ldw)
    R = torch.full((B, NB + 2, ldr), SENT, dtype=torch.float32, device=DEV)
    Wn = torch.full((B, NB, ldw), SENT, dtype=torch.float32, device=DEV)
    info = torch.zeros(B, dtype=torch.int32, device=DEV)
    check(lib.roma_chol_step(A.data_ptr(), lda, A.stride(0), n, ncols, j, nb, W.data_ptr(), ldw, W.stride(0), R.data_ptr(), ldr, R.stride(0),
                             None if last else Wn.data_ptr(), ldw, Wn.stride(0), info.data_ptr(), e, B, _st()), "step")
    torch.cuda.synchronize()
    A, R, Wn = A.cpu(), R.cpu(), Wn.cpu()
    Rref, Tref, Lref, Wnref = G.chol_step_ref(A32, n, ncols, j, nb, W32)
    bR, bT = G.step_bounds(A32, n, ncols, j, nb, W32)
    # R over its nb x (ncols - e) extent; nothing else of the buffer
    _within(R[:, :nb, :ncols - e], Rref, bR, f"{name} R")
    outside = torch.ones_like(R, dtype=torch.bool)
    outside[:, :nb, :ncols - e] = False
    assert bool((R[outside] == SENT).all())
    # the trailing region: tiles (I, J >= I) updated, tiles below the block diagonal and everything else exactly as they were
    touched = torch.zeros_like(A, dtype=torch.bool)
    nbn = min(NB, n - e)
    for I, i0 in enumerate(range(e, n, NB)):
        i1 = min(i0 + NB, n)
        touched[:, i0:i1, i0:ncols] = True
        got, ref, bnd = A[:, i0:i1, i0:ncols], Tref[:, i0 - e:i1 - e, i0 - e:], bT[:, i0 - e:i1 - e, i0 - e:]
        if I == 0:                                                    # next diagonal block: factored in place; its strict upper triangle is
            keep = torch.ones(i1 - i0, ncols - i0, dtype=torch.bool)  # not part of the contract (nothing reads it)
            keep[:nbn, :nbn] = False
            _within(got[:, keep], ref[:, keep], bnd[:, keep], f"{name} tile row 0")
        else:
            _within(got, ref, bnd, f"{name} tile row {I}")
    assert torch.equal(A[~touched], A0[~touched])                     # rows above, columns left, tiles I > J, row n, padding
    if not last:
        L, Wi, tolL, tolW = G.factor_bounds(Tref[:, :nbn, :nbn], bT[:, :nbn, :nbn])
        eL = (torch.tril(A[:, e:e + nbn, e:e + nbn]).double() - L).abs().amax(dim=(1, 2))
        eW = (Wn[:, :nbn, :nbn].double() - Wi).abs().amax(dim=(1, 2))
        print(f"{name}: nbn={nbn} |L - ref| {eL.tolist()} (bound {tolL.tolist()}), |Wn - ref| {eW.tolist()} (bound {tolW.tolist()})")
        assert bool((eL <= tolL).all()) and bool((eW <= tolW).all())
        assert float((L - Lref).abs().max()) == 0.0 and float((Wi - Wnref).abs().max()) == 0.0     # the bounds' L is chol_step_ref's
        assert float(torch.triu(Wn[:, :nbn, :nbn], 1).abs().max() if nbn > 1 else 0.0) == 0.0
        outside = torch.ones_like(Wn, dtype=torch.bool)
        outside[:, :nbn, :nbn] = False
        assert bool((Wn[outside] == SENT).all())
    else:
        assert bool((Wn == SENT).all())
    assert int(info.abs().max()) == 0


# ---- 4. roma_chol_subst_step ------------------------------------------------------------------------------------------------------
def _subst_cases():
    cases = []
    for n in (200, 128):
        S = len(G.blocks(n))
        for s in range(S):
            cases += [(n, +1, s, 24, 0), (n, -1, s, 24, 0), (n, -1, s, 24, 1)]          # every source block, both directions, both layouts
    for m in (1, 64, 65, 130):                                                          # one, two, three column tiles; m % 4 != 0; m = 1
        cases += [(200, +1, 1, m, 0), (200, -1, 2, m, 0), (200, -1, 2, m, 1)]
    return cases


@pytest.fixture(scope="module")
def synthetic_factor():
    """n -> the fp64 Cholesky factor of a well-conditioned K (B = 2), computed once."""
    out = {}
    for n in (200, 128):
        K, _ = G.well_conditioned_system(2, n, 1, seed=40 + n)
        out[n] = torch.linalg.cholesky(K.double())
    return out


@pytest.mark.parametrize("n,direction,s,m,in_panel", _subst_cases())
def test_subst_step_against_its_definition(synthetic_factor, n, direction, s, m, in_panel):
    lib, check = _abi()
    B, ldx = 2, m + 3
    Lf = synthetic_factor[n]
    S = len(G.blocks(n))
    rhs = torch.randn(B, n, m, generator=torch.Generator().manual_seed(7 * n + 13 * s + m)).float()
    Wall, Pall = G.pack_panels(Lf, n, m, rhs=rhs if in_panel else None)
    Wd, Pd = Wall.float().to(DEV), Pall.float().to(DEV)
    P0 = Pd.cpu()
    # the reference works on what the kernel is given: the fp32-rounded panels and inverse factors
    L32, _ = G.unpack_panels(Wall, Pd.cpu(), n, m)
    Wb = [Wd[:, k, :e - j, :e - j].cpu().double() for k, (j, e) in enumerate(G.blocks(n))]
    Xs, Tref = G.subst_step_ref(direction, L32, Wb, rhs, s)
    js, es = s * NB, min((s + 1) * NB, n)
    X = torch.full((B, n + 1, ldx), SENT, dtype=torch.float32, device=DEV)
    if in_panel:                                                      # T = R, the layout roma_chol_step leaves Y in
        T, sTb, sTs, ldt = Pd, Pd.stride(0), Pd.stride(1), n + m
    else:                                                             # a right-hand side of its own, rows ldt > m apart
        ldt = m + 5
        T = _padded(rhs, S * NB, ldt)
        T0 = T.cpu()
        sTb, sTs = T.stride(0), NB * ldt
    check(lib.roma_chol_subst_step(direction, Wd[:, s].data_ptr(), NB, Wd.stride(0), Pd.data_ptr(), Pd.stride(0), Pd.stride(1), n + m,
                                   T.data_ptr(), sTb, sTs, ldt, in_panel, X.data_ptr(), ldx, X.stride(0), n, m, NB, s, B, _st()), "subst")
    torch.cuda.synchronize()
    X, T = X.cpu(), T.cpu()
    absW = Wb[s].abs() if direction > 0 else Wb[s].abs().transpose(1, 2)
    PX = absW @ rhs[:, js:es].double().abs()                          # >= |X_s|
    _within(X[:, js:es, :m], Xs, (es - js + 2) * G.U32 * PX, "X_s")
    outside = torch.ones_like(X, dtype=torch.bool)
    outside[:, js:es, :m] = False
    assert bool((X[outside] == SENT).all())                           # rows of X outside block s, the pitch padding
    # T afterwards: the block rows the step updates, within u |T| + 3 (w_s + 2) u |L piece| (|W_s| |T_s|) (the computed X_s enters a
    # second product, as in gp_ref.step_bounds); every other element of the buffer bit for bit
    rows = range(0, js) if direction < 0 else range(es, n)
    absL = (L32[:, js:es, :js].abs().transpose(1, 2) if direction < 0 else L32[:, es:, js:es].abs())
    bT = torch.zeros(B, n, m, dtype=torch.float64)
    if len(rows):
        bT[:, rows.start:rows.stop] = G.U32 * rhs[:, rows.start:rows.stop].double().abs() + 3 * (es - js + 2) * G.U32 * (absL @ PX)
    if in_panel:
        _, Tgot = G.unpack_panels(Wall, T, n, m)
        untouched = torch.ones_like(T, dtype=torch.bool)
        for k, (j, e) in enumerate(G.blocks(n)):
            if j in rows:
                untouched[:, k, :e - j, n - e:n - e + m] = False
        assert torch.equal(T[untouched], P0[untouched])               # the L part of EVERY panel, block rows >= s, the unused corners
    else:
        Tgot = T[:, :n, :m].double()
        untouched = torch.ones_like(T, dtype=torch.bool)
        if len(rows):
            untouched[:, rows.start:rows.stop, :m] = False
        assert torch.equal(T[untouched], T0[untouched])
        assert torch.equal(Pd.cpu(), P0)                              # the factor is read only
    _within(Tgot, Tref, bT, "T")                                      # bound 0 outside the updated rows: exact there


# ---- 5. spd_solve as a whole ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 128, 129, 192])
def test_spd_solve_shape_sweep(n):
    ops = _ops()
    for m in (1, 7, 64, 65):
        for B in (1, 3):
            K, F = G.well_conditioned_system(B, n, m, seed=n * 100 + m)
            Kd = K.to(DEV)
            for form in ("full", "broadcast"):
                Fh = F if form == "full" else F[:1].expand(B, -1, -1)
                Fd = F.to(DEV) if form == "full" else F[:1].to(DEV).expand(B, -1, -1)
                ref = G.solve64(K, Fh)
                X = ops.spd_solve(Kd, Fd)
                assert X.shape == (B, n, m)
                err, bar = float((X.cpu().double() - ref).abs().max()), 2e-5 * float(ref.abs().max())
                assert err < bar, (n, m, B, form, err, bar)


# Measured on MI355X (forward = max|X - ref| / max|ref|, backward = |K X - F|_F / (|K|_F |X|_F), both against / in fp64 on the
# fp32-stored K; cond_2 of each case: gp_ref.ILL_CASES; "fp32" = LAPACK's fp32 Cholesky solve on the host):
#            forward: kernel   fp32        backward: kernel   fp32        refine=1: forward   backward
#   c200              9.01e-5  1.67e-4               6.79e-9  6.35e-9               4.81e-8   1.06e-9
#   c256              2.87e-4  1.99e-4               5.92e-9  5.20e-9               1.92e-7   9.46e-10
#   c321              4.62e-4  3.48e-4               5.28e-9  5.50e-9               4.41e-7   8.29e-10
# The 4 x margin covers the kernel's 1-ulp rcp / rsq pivots and its different summation order; nothing larger is explained by the design.
@pytest.mark.parametrize("name", list(G.ILL_CASES))
def test_spd_solve_ill_conditioned_against_the_fp32_reference(name):
    ops = _ops()
    K, F = G.ill_system(name)
    ref = G.solve64(K, F)
    f32, b32 = G.solve_errors(G.fp32_solve(K, F), K, F, ref)
    Kd, Fd = K.to(DEV), F.to(DEV)
    fk, bk = G.solve_errors(ops.spd_solve(Kd, Fd), K, F, ref)
    fk1, bk1 = G.solve_errors(ops.spd_solve(Kd, Fd, refine=1), K, F, ref)
    print(f"{name}: forward kernel {fk:.3e} fp32 {f32:.3e} | backward kernel {bk:.3e} fp32 {b32:.3e} | refine=1 forward {fk1:.3e} backward {bk1:.3e}")
    assert fk <= 4 * f32
    assert bk <= 4 * b32
    assert fk1 <= fk


def test_spd_solve_items_are_independent_and_inputs_untouched():
    ops = _ops()
    K, F = G.well_conditioned_system(3, 129, 7, seed=77)
    Kd, Fd = K.to(DEV), F.to(DEV)
    K0, F0 = Kd.clone(), Fd.clone()
    X = ops.spd_solve(Kd, Fd)
    assert torch.equal(ops.spd_solve(Kd, Fd), X)                      # two identical calls
    for b in range(3):
        assert torch.equal(ops.spd_solve(Kd[b:b + 1], Fd[b:b + 1])[0], X[b]), b
    X1 = ops.spd_solve(Kd, Fd, refine=1)
    for b in range(3):
        assert torch.equal(ops.spd_solve(Kd[b:b + 1], Fd[b:b + 1], refine=1)[0], X1[b]), b
    Fb = Fd[:1].expand(3, -1, -1)
    ops.spd_solve(Kd, Fb)
    assert torch.equal(Kd, K0) and torch.equal(Fd, F0)                # spd_solve works on a copy


# ---- 6. the not-SPD record --------------------------------------------------------------------------------------------------------
def _blocked_solve(K, F):
    """The launch sequence of ops._spd_solve (refine = 0) through the ABI; returns (X, info)."""
    lib, check = _abi()
    B, n, _ = K.shape
    m = F.shape[2]
    A = torch.cat((K, F), dim=2).contiguous()
    steps = G.blocks(n)
    S = len(steps)
    W = torch.zeros((B, S, NB, NB), dtype=torch.float32, device=K.device)
    Rall = torch.zeros((B, S, NB, n + m), dtype=torch.float32, device=K.device)
    info = torch.zeros((B,), dtype=torch.int32, device=K.device)
    check(lib.roma_chol_diag_block(A.data_ptr(), n + m, A.stride(0), W.data_ptr(), NB, W.stride(0), steps[0][1], B, info.data_ptr(), 0, _st()),
          "diag")
    for s, (j, e) in enumerate(steps):
        check(lib.roma_chol_step(A.data_ptr(), n + m, A.stride(0), n, n + m, j, e - j, W[:, s].data_ptr(), NB, W.stride(0), Rall[:, s].data_ptr(),
                                 n + m, Rall.stride(0), None if s + 1 == S else W[:, s + 1].data_ptr(), NB, W.stride(0), info.data_ptr(),
                                 NB * (s + 1), B, _st()), "step")
    X = torch.zeros((B, n, m), dtype=torch.float32, device=K.device)
    for s in range(S - 1, -1, -1):
        check(lib.roma_chol_subst_step(-1, W[:, s].data_ptr(), NB, W.stride(0), Rall.data_ptr(), Rall.stride(0), Rall.stride(1), n + m,
                                       Rall.data_ptr(), Rall.stride(0), Rall.stride(1), n + m, 1, X.data_ptr(), m, X.stride(0), n, m, NB, s, B,
                                       _st()), "subst")
    torch.cuda.synchronize()
    return X, info.cpu().tolist()


@pytest.fixture(scope="module")
def spd200():
    K, F = G.well_conditioned_system(3, 200, 8, seed=5)
    return K.to(DEV), F.to(DEV)


@pytest.mark.parametrize("pivots,expect", [((5,), 6), ((130,), 131), ((195,), 196), ((70, 195), 71), ((195, 70), 71), ((0,), 1), ((64,), 65),
                                           ((199,), 200)])
def test_info_is_the_first_failing_pivot_plus_one(spd200, pivots, expect):
    K, F = spd200
    bad = K.clone()
    for p in pivots:
        bad[1, p, p] = -5.0
    X, info = _blocked_solve(bad, F)
    assert info == [0, expect, 0]
    good, ginfo = _blocked_solve(K, F)
    assert ginfo == [0, 0, 0]
    assert torch.equal(X[0], good[0]) and torch.equal(X[2], good[2])   # the other items of the batch are unaffected
    assert torch.equal(good, _ops().spd_solve(K, F))                  # and this helper IS spd_solve's sequence


@pytest.mark.parametrize("p", [3, 130, 195])
def test_info_records_a_nan_on_the_diagonal(spd200, p):
    K, F = spd200
    bad = K.clone()
    bad[2, p, p] = float("nan")
    X, info = _blocked_solve(bad, F)                                  # the kernel clamps and carries on: the call returns
    assert info == [0, 0, p + 1]
    good, _ = _blocked_solve(K, F)
    assert torch.equal(X[0], good[0]) and torch.equal(X[1], good[1])


def test_spd_solve_error_names_block_step_and_pivot(spd200):
    from roma_amd._lib import RomaHipError
    K, F = spd200
    bad = K.clone()
    bad[1, 195, 195] = -5.0
    with pytest.raises(RomaHipError, match="matrix 1 .*block step 3, pivot 3 "):
        _ops().spd_solve(bad, F, check="now")
    bad[0, 70, 70] = -5.0
    with pytest.raises(RomaHipError, match="matrix 0 .*block step 1, pivot 6 "):
        _ops().spd_solve(bad, F, check="now")


# ---- 7. cos_kernel ----------------------------------------------------------------------------------------------------------------
def _randn(shape, seed, dtype=torch.float32):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dtype)


def _cos_check(x, y, what, diag_self=False, **kw):
    """ops.cos_kernel on device copies of x, y against cos_kernel_ref of the same stored values: 2e-6, and 6e-6 on the diagonal of a
    self-kernel matrix (c ~ 1 there, and exp((c-1)/T) amplifies the fp32 rounding of the result by 1/T = 5 — the existing bound)."""
    out = _ops().cos_kernel(x.to(DEV), y.to(DEV), **kw)
    ref = G.cos_kernel_ref(x, y, **kw)
    assert out.shape == ref.shape and out.dtype == torch.float32
    assert bool(torch.isfinite(out).all())
    err = (out.cpu().double() - ref).abs()
    N, M = err.shape[1:]
    eye = torch.eye(N, M, dtype=torch.bool)
    print(f"{what}: off-diagonal {float(err[:, ~eye].max()) if (~eye).any() else 0.0:.2e}, diagonal {float(err[:, eye].max()):.2e}")
    assert not (~eye).any() or float(err[:, ~eye].max()) < 2e-6
    assert float(err[:, eye].max()) < (6e-6 if diag_self else 2e-6)
    return out


@pytest.mark.parametrize("D", [16, 48, 64, 80, 144])
def test_cos_kernel_channel_counts(D):
    x, y = _randn((2, 70, D), D), _randn((2, 70, D), D + 1)
    _cos_check(x, y, f"D={D}")
    _cos_check(x, x, f"D={D} self", diag_self=True, diag_add=0.1)


@pytest.mark.parametrize("N,M", [(1, 1), (65, 1), (1, 65), (70, 130), (129, 64), (64, 128)])
def test_cos_kernel_partial_tiles(N, M):
    _cos_check(_randn((2, N, 64), N), _randn((2, M, 64), 1000 + M), f"{N}x{M}")


@pytest.mark.parametrize("N,M", [(70, 130), (130, 70)])
def test_cos_kernel_diag_add_on_a_non_square_output(N, M):
    x, y = _randn((2, N, 64), 3), _randn((2, M, 64), 4)
    with_d = _cos_check(x, y, f"{N}x{M} diag_add", diag_add=0.1)
    without = _ops().cos_kernel(x.to(DEV), y.to(DEV))
    eye = torch.eye(N, M, dtype=torch.bool, device=DEV)
    assert torch.equal(with_d[:, ~eye], without[:, ~eye])             # nowhere else
    assert torch.equal(with_d[:, eye], without[:, eye] + 0.1)         # exactly where n == m: one fp32 addition


@pytest.mark.parametrize("xdt,ydt", [(torch.float16, torch.float16), (torch.bfloat16, torch.bfloat16), (torch.float16, torch.float32),
                                     (torch.float32, torch.bfloat16)])
def test_cos_kernel_16_bit_rows(xdt, ydt):
    x, y = _randn((2, 70, 80), 5, xdt), _randn((2, 130, 80), 6, ydt)  # the reference is fed the rounded values
    _cos_check(x, y, f"{xdt} x {ydt}")
    _cos_check(x, x, f"{xdt} self", diag_self=True, diag_add=0.1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_cos_kernel_strided_rows_against_fp64(dtype):
    ops = _ops()
    buf = _randn((2, 7, 10, 200), 8, dtype).to(DEV)                    # a wider channels-last buffer; the features are channels 8 .. 72
    x = buf[..., 8:72].reshape(2, 70, 64)
    y = buf[..., 104:168].reshape(2, 70, 64)
    assert x.data_ptr() == buf.data_ptr() + 8 * buf.element_size() and x.stride(1) == 200
    assert ops._rows(x)[1] == 200 and ops._rows(x)[0].data_ptr() == x.data_ptr()     # read in place, not copied
    out = ops.cos_kernel(x, y, diag_add=0.1)
    err = (out.cpu().double() - G.cos_kernel_ref(x, y, diag_add=0.1)).abs()
    print(f"strided {dtype}: {float(err.max()):.2e}")
    assert float(err.max()) < 2e-6


@pytest.mark.parametrize("shift", [0, 1, 2])
def test_cos_kernel_batch_shift(shift):
    x, y = _randn((3, 70, 64), 9), _randn((3, 40, 64), 10)
    out = _cos_check(x, y, f"shift {shift}", batch_shift=shift)
    explicit = _ops().cos_kernel(x.to(DEV), y.roll(-shift, 0).to(DEV))
    assert torch.equal(out, explicit)


def test_cos_kernel_scaled_rows():
    sx = torch.logspace(-3, 3, 70)[None, :, None]
    sy = torch.logspace(3, -3, 130)[None, :, None]
    _cos_check(_randn((2, 70, 64), 11) * sx, _randn((2, 130, 64), 12) * sy, "scaled")   # eps is visible at the small end: the reference carries it


def test_cos_kernel_zero_rows():
    x, y = _randn((2, 70, 64), 13), _randn((2, 70, 64), 14)
    x[0, 3] = 0
    y[1, 5] = 0
    y[0, 69] = 0
    out = _cos_check(x, y, "zero rows").cpu()
    v = torch.exp(torch.tensor(-1 / 0.2, dtype=torch.float64)).float()
    for line in (out[0, 3], out[1, :, 5], out[0, :, 69]):              # exp(-1/T) along the whole row / column
        assert bool((line == line[0]).all()) and abs(float(line[0] - v)) < 1e-9


def test_cos_kernel_argument_errors_launch_nothing():
    from roma_amd import _lib
    lib = _lib.load()
    B, N, M = 3, 8, 8
    x = torch.ones(B, N, 96, device=DEV)
    K = torch.full((B, N, M), SENT, device=DEV)

    def call(D, dtype, xp, yp, shift, xptr=None):
        return lib.roma_cos_kernel(xptr or x.data_ptr(), x.data_ptr(), K.data_ptr(), B, N, M, D, dtype, xp, yp, shift, 0.2, 1e-6, 0.0, _st())

    assert call(24, _lib.ROMA_F32, 96, 96, 0) == _lib.ROMA_E_SHAPE and b"multiple of 16" in lib.roma_last_error()
    assert call(32, _lib.ROMA_F32, 16, 96, 0) == _lib.ROMA_E_SHAPE                  # pitch smaller than D
    assert call(32, _lib.ROMA_F32, 34, 96, 0) == _lib.ROMA_E_ALIGN                  # rows not 16-byte aligned
    assert call(32, _lib.ROMA_F16, 96, 36, 0) == _lib.ROMA_E_ALIGN                  # 16-bit rows: pitch must be a multiple of 8
    assert call(32, _lib.ROMA_F32, 96, 96, 0, xptr=x.data_ptr() + 4) == _lib.ROMA_E_ALIGN
    assert call(32, _lib.ROMA_F32, 96, 96, B) == _lib.ROMA_E_ARG and b"y_batch_shift" in lib.roma_last_error()
    assert call(32, _lib.ROMA_F32, 96, 96, -1) == _lib.ROMA_E_ARG
    assert call(32, 3, 96, 96, 0) == _lib.ROMA_E_DTYPE
    torch.cuda.synchronize()
    assert bool((K == SENT).all())                                    # nothing was launched
    assert call(32, _lib.ROMA_F32, 96, 96, B - 1) == 0                # the same call with legal arguments runs
    torch.cuda.synchronize()
    assert bool((K != SENT).all())


# ---- 8. GP.posterior_rows, small --------------------------------------------------------------------------------------------------
def _gp(sigma):
    import roma_amd.matcher as M
    return H.load_recipe_weights(M.GP(32, sigma_noise=sigma), "gp.stage.", gains={"pos_conv": 4.0}).to(DEV)


def _gp_rows(B=4, n=117, seed=21):
    xs = G.clustered_features(B, n, 64, 9, 0.05, seed).float()
    ys = G.clustered_features(B, n, 64, 9, 0.05, seed + 1).float()
    return xs, ys


# Measured on MI355X, max|mu - mu_fp64| (h2 x w2 = 9 x 13, B = 4, D = 64, gp_dim = 32, clustered features):
#   sigma = 0.1:   fast path 2.03e-6, fp32 torch 1.96e-6 (|mu| max 0.08)      sigma = 1e-3:  fast path 1.64e-4, fp32 torch 1.60e-4 (|mu| max 0.75)
@pytest.mark.parametrize("sigma", [0.1, 1e-3])
def test_posterior_rows_fast_path_against_fp64(sigma):
    gp = _gp(sigma)
    xs, ys = _gp_rows()
    fast = gp.posterior_rows(xs.to(DEV), ys.to(DEV), 9, 13).cpu().double()
    exact = gp.posterior_rows(xs.to(DEV), ys.to(DEV), 9, 13, fp64=True).cpu().double()
    assert fast.shape == (4, 117, 32)
    # the same computation with fp32 torch on the host: cos in fp32, fp32 Cholesky solve, fp64-accumulated product
    basis = gp.basis(1, 9, 13, DEV).cpu()

    def cosk(u, v):
        g = torch.einsum("bnd,bmd->bnm", u, v) / (u.norm(dim=-1)[..., None] * v.norm(dim=-1)[:, None] + 1e-6)
        return ((g - 1.0) / gp.K.T).exp()

    Z = G.fp32_solve(cosk(ys, ys) + sigma * torch.eye(117), basis.expand(4, -1, -1).contiguous())
    mu32 = cosk(xs, ys).double() @ Z.double()
    ek, e32 = float((fast - exact).abs().max()), float((mu32 - exact).abs().max())
    print(f"sigma={sigma}: |mu| max {float(exact.abs().max()):.2f}; fast path {ek:.3e}, fp32 torch {e32:.3e}")
    assert ek <= 4 * e32


def test_posterior_rows_swapped_pair_form_and_out():
    gp = _gp(0.1)
    xs, _ = _gp_rows()
    xs = xs.to(DEV)
    B = xs.shape[0]
    explicit = gp.posterior_rows(xs, xs.roll(-(B // 2), 0).contiguous(), 9, 13)
    swapped = gp.posterior_rows(xs, None, 9, 13, batch_shift=B // 2)
    assert float((swapped - explicit).abs().max()) < 1e-5
    for ys, shift in ((None, B // 2), (xs.roll(-1, 0).contiguous(), 0)):
        out = torch.full((B, 117, 32), SENT, device=DEV)
        ret = gp.posterior_rows(xs, ys, 9, 13, batch_shift=shift, out=out)
        assert ret.data_ptr() == out.data_ptr()
        assert torch.equal(out, gp.posterior_rows(xs, ys, 9, 13, batch_shift=shift))
