"""CPU self-checks of the fp64 GP-stage references (tests/gp_ref.py): they must be right before a kernel is measured against them."""
import pytest
import torch

from tests import gp_ref as G

torch.set_grad_enabled(False)


@pytest.mark.parametrize("n,m", [(200, 24), (128, 5), (40, 3), (1, 2)])
def test_chained_step_references_reproduce_the_fp64_solve(n, m):
    K, F = G.well_conditioned_system(2, n, m, seed=11)
    X, Lfull, Wb, Y = G.blocked_solve_ref(K, F)
    ref = G.solve64(K, F)
    assert float((X - ref).abs().max()) < 1e-10
    assert float((Lfull - torch.linalg.cholesky(K.double())).abs().max()) < 1e-10
    # forward substitution with a new right-hand side, then back: the refinement path's two sweeps
    g = torch.randn(2, n, m, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    T, Yg = g, torch.zeros_like(g)
    for s in range(len(Wb)):
        Ys, T = G.subst_step_ref(+1, Lfull, Wb, T, s)
        Yg[:, s * G.NB:s * G.NB + Ys.shape[1]] = Ys
    T, Xg = Yg, torch.zeros_like(g)
    for s in range(len(Wb) - 1, -1, -1):
        Xs, T = G.subst_step_ref(-1, Lfull, Wb, T, s)
        Xg[:, s * G.NB:s * G.NB + Xs.shape[1]] = Xs
    assert float((Xg - G.solve64(K, g)).abs().max()) < 1e-10


def test_state_before_step_is_the_schur_complement():
    K, F = G.well_conditioned_system(1, 200, 7, seed=2)
    A = G.state_before_step(K, F, 128)
    Kd, Fd = K.double(), F.double()
    S = Kd[:, 128:, 128:] - Kd[:, 128:, :128] @ torch.linalg.solve(Kd[:, :128, :128], Kd[:, :128, 128:])
    assert float((A[:, 128:, 128:200] - S).abs().max()) < 1e-12
    assert torch.equal(A[:, :64], torch.cat((Kd, Fd), dim=2)[:, :64])          # rows above are left as they were


@pytest.mark.parametrize("n,m", [(200, 24), (128, 5), (40, 3)])
def test_pack_panels_round_trips(n, m):
    K, F = G.well_conditioned_system(2, n, m, seed=3)
    L = torch.linalg.cholesky(K.double())
    Wall, Pall = G.pack_panels(L, n, m, rhs=F)
    L2, rhs = G.unpack_panels(Wall, Pall, n, m)
    assert float((L2 - L).abs().max()) < 1e-12 and torch.equal(rhs, F.double())
    for k, (j, e) in enumerate(G.blocks(n)):                                   # nothing outside the documented extents
        assert float(Pall[:, k, e - j:].abs().max() if e - j < G.NB else 0.0) == 0.0
        assert float(Pall[:, k, :, n - e + m:].abs().max() if n - e + m < n + m else 0.0) == 0.0
        assert float(Wall[:, k, e - j:].abs().max() if e - j < G.NB else 0.0) == 0.0
    Wall0, Pall0 = G.pack_panels(L, n, m)
    assert float(Pall0[:, -1].abs().max()) == 0.0                              # the last panel has no L part, and no rhs was given


def test_cos_kernel_ref_semantics():
    g = torch.Generator().manual_seed(0)
    x, y = torch.randn(3, 5, 16, generator=g), torch.randn(3, 7, 16, generator=g)
    K = G.cos_kernel_ref(x, y, T=0.2, eps=1e-6, diag_add=0.25, batch_shift=2)
    for b in range(3):
        for n in range(5):
            for m in range(7):
                a, c = x[b, n].double(), y[(b + 2) % 3, m].double()
                v = torch.exp((a @ c / (a.norm() * c.norm() + 1e-6) - 1) / 0.2) + (0.25 if n == m else 0.0)
                assert abs(float(K[b, n, m] - v)) < 1e-14
    # 16-bit rows are widened exactly; a zero row gives exp(-1/T)
    h = x.half()
    assert torch.equal(G.cos_kernel_ref(h, h), G.cos_kernel_ref(h.float(), h.float()))
    z = x.clone()
    z[1, 2] = 0
    Kz = G.cos_kernel_ref(z, y)
    assert float((Kz[1, 2] - torch.exp(torch.tensor(-5.0, dtype=torch.float64))).abs().max()) == 0.0


def test_cos_kernel_ref_matches_the_oracle():
    from oracle import roma_oracle as O
    g = torch.Generator().manual_seed(1)
    x, y = torch.randn(2, 33, 64, generator=g), torch.randn(2, 21, 64, generator=g)
    assert float((G.cos_kernel_ref(x, y) - O.cos_kernel(x, y).double()).abs().max()) < 2e-6


@pytest.mark.parametrize("name", list(G.ILL_CASES))
def test_ill_conditioned_cases_are_in_the_range_of_real_features(name):
    K, F = G.ill_system(name)
    cond = G.single_thread(torch.linalg.cond, K.double())
    print(name, [f"{float(c):.2e}" for c in cond])
    assert float(cond.min()) > 5e3 and float(cond.max()) < 1e5
    Kw, _ = G.well_conditioned_system(2, 200, 1, seed=0)
    assert float(G.single_thread(torch.linalg.cond, Kw.double()).max()) < 1e2


def test_clustered_features_are_unit_rows_and_deterministic():
    x = G.clustered_features(2, 50, 64, 5, 0.05, 3)
    assert x.dtype == torch.float64 and float((x.norm(dim=-1) - 1).abs().max()) < 1e-14
    assert torch.equal(x, G.clustered_features(2, 50, 64, 5, 0.05, 3))
    assert float((x[:, 0] * x[:, 5]).sum(-1).min()) > 0.9                      # same cluster: near-duplicates
