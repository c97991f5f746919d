"""Plain fp64 references of the GP stage (CosKernel, the blocked Cholesky solve), written from the contracts in include/roma_hip.h.
torch on the CPU only: importable and testable without a GPU (tests/test_gp_ref.py); the GPU comparisons are tests/test_gp_stage.py."""
import torch

NB = 64                                                            # the block size of the blocked solve
U32 = 2.0 ** -24                                                   # unit roundoff of fp32


def solve64(K, F):
    """fp64 reference solve on ONE host thread: multithreaded oneMKL getrf hangs on the GPU boxes' host CPUs (see
    oracle._inv_single_thread)."""
    nt = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return torch.linalg.solve(K.double(), F.double())
    finally:
        torch.set_num_threads(nt)


def single_thread(fn, *args):
    """fn(*args) on one host thread (the fp64 / fp32 LAPACK references; same reason as solve64)."""
    nt = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return fn(*args)
    finally:
        torch.set_num_threads(nt)


def cos_kernel_ref(x, y, T=0.2, eps=1e-6, diag_add=0.0, batch_shift=0):
    """K[b,n,m] = exp((<x_n,y_m>/(|x_n||y_m| + eps) - 1)/T) in fp64; x[b] meets y[(b + batch_shift) % B]; diag_add where n == m.
    x, y: (B,N,D) / (B,M,D) of any float dtype, widened exactly."""
    a = x.detach().cpu().double()
    c = y.detach().cpu().double()
    B = a.shape[0]
    if batch_shift % B:
        c = c.roll(-(batch_shift % B), 0)                          # c[b] = y[(b + shift) % B]
    g = torch.einsum("bnd,bmd->bnm", a, c) / (a.norm(dim=-1)[:, :, None] * c.norm(dim=-1)[:, None, :] + eps)
    K = ((g - 1.0) / T).exp()
    N, M = K.shape[1:]
    d = min(N, M)
    K[:, torch.arange(d), torch.arange(d)] += diag_add
    return K


def chol_step_ref(A, n, ncols, j, nb, W):
    """One fused forward step on the augmented matrix A (B, n, >= ncols) fp64, block rows [j, j+nb), W (B,nb,nb) the inverse factor
    of their diagonal block.  Returns (R, trailing, L, Linv): R = W A[j:e, e:ncols]; trailing = A[e:n, e:ncols] - R[:, :n-e]^T R
    (the WHOLE region; the kernel keeps only the 64 x 64 tiles on or right of the diagonal up to date); L / Linv = the Cholesky
    factor (lower) of the next diagonal block trailing[:nbn, :nbn], nbn = min(64, n - e), and its inverse (None if e == n)."""
    e = j + nb
    A = A.double()
    R = W.double() @ A[:, j:e, e:ncols]
    trailing = A[:, e:n, e:ncols] - R[:, :, :n - e].transpose(1, 2) @ R
    if e == n:
        return R, trailing, None, None
    nbn = min(NB, n - e)
    L = torch.linalg.cholesky(trailing[:, :nbn, :nbn])
    return R, trailing, L, torch.linalg.inv(L)


def subst_step_ref(direction, Lfull, Wblocks, T, s, nb=NB):
    """One substitution step with the finished factor Lfull (B,n,n), Wblocks[k] = (B,w_k,w_k) the inverse of diagonal block k,
    right-hand side T (B,n,m).  Returns (X_s, T afterwards):
      direction < 0:  X_s = W_s^T T_s;  T_i -= L[block s, block i]^T X_s  for i < s
      direction > 0:  X_s = W_s T_s;    T_i -= L[block i, block s] X_s    for i > s"""
    n = Lfull.shape[1]
    js, es = s * nb, min((s + 1) * nb, n)
    L, T = Lfull.double(), T.double().clone()
    Ws = Wblocks[s].double()
    if direction < 0:
        Xs = Ws.transpose(1, 2) @ T[:, js:es]
        T[:, :js] -= L[:, js:es, :js].transpose(1, 2) @ Xs
    else:
        Xs = Ws @ T[:, js:es]
        T[:, es:] -= L[:, es:, js:es] @ Xs
    return Xs, T


def blocks(n, nb=NB):
    return [(j, min(j + nb, n)) for j in range(0, n, nb)]


def pack_panels(Lfull, n, m, nb=NB, rhs=None):
    """The layout roma_chol_step leaves behind: Wall (B,S,nb,nb), Wall[:, k] = inv(L_kk) in the top-left corner, zero elsewhere;
    Pall (B,S,nb,n+m), the first n - e_k columns of panel k = L[e_k:, block k]^T.  rhs (B,n,m), if given, is placed in the
    t_in_panel layout: the share of block row k starts at column n - e_k of panel k."""
    B = Lfull.shape[0]
    S = len(blocks(n, nb))
    Wall = torch.zeros(B, S, nb, nb, dtype=torch.float64)
    Pall = torch.zeros(B, S, nb, n + m, dtype=torch.float64)
    for k, (j, e) in enumerate(blocks(n, nb)):
        Wall[:, k, :e - j, :e - j] = torch.linalg.inv(Lfull[:, j:e, j:e].double())
        Pall[:, k, :e - j, :n - e] = Lfull[:, e:, j:e].double().transpose(1, 2)
        if rhs is not None:
            Pall[:, k, :e - j, n - e:n - e + m] = rhs[:, j:e].double()
    return Wall, Pall


def unpack_panels(Wall, Pall, n, m, nb=NB):
    """Inverse of pack_panels: (Lfull, rhs) from the packed factor (the diagonal blocks from inv(W_k))."""
    B = Wall.shape[0]
    L = torch.zeros(B, n, n, dtype=torch.float64)
    rhs = torch.zeros(B, n, m, dtype=torch.float64)
    for k, (j, e) in enumerate(blocks(n, nb)):
        L[:, j:e, j:e] = torch.linalg.inv(Wall[:, k, :e - j, :e - j].double())
        L[:, e:, j:e] = Pall[:, k, :e - j, :n - e].double().transpose(1, 2)
        rhs[:, j:e] = Pall[:, k, :e - j, n - e:n - e + m].double()
    return L, rhs


def clustered_features(B, n, D, clusters, noise, seed):
    """normalize(centre[i % clusters] + noise * randn), fp64: near-duplicate rows, so the kernel matrix has a few large eigenvalues,
    and with a small sigma on the diagonal small ones — the ill-conditioned systems real features give."""
    g = torch.Generator().manual_seed(seed)
    centres = torch.randn(B, clusters, D, generator=g, dtype=torch.float64)
    x = centres[:, torch.arange(n) % clusters] + noise * torch.randn(B, n, D, generator=g, dtype=torch.float64)
    return torch.nn.functional.normalize(x, dim=-1)


# Ill-conditioned solver cases: name -> (n, clusters, noise, sigma), B = 3, D = 64, T = 0.2, seed 7, m = 33.  cond_2 of the fp32-stored
# K = cos_kernel_ref(x, x) + sigma I, evaluated in fp64 (tests/test_gp_ref.py asserts the range), per batch item:
#   c200: 1.07e4 1.05e4 8.99e3      c256: 2.30e4 2.29e4 2.26e4      c321: 4.09e4 4.24e4 4.23e4
# — the 1e4 .. 1e5 the solver's comments give for real features.  The well-conditioned recipe below has cond < 1e2.
ILL_CASES = {"c200": (200, 8, 0.05, 1e-3), "c256": (256, 10, 0.02, 1e-3), "c321": (321, 12, 0.02, 5e-4)}


def ill_system(name, m=33):
    """(K, F) fp32 of an ILL_CASES entry: K (3,n,n), F (3,n,m) ~ N(0,1)."""
    n, clusters, noise, sigma = ILL_CASES[name]
    x = clustered_features(3, n, 64, clusters, noise, 7)
    K = (cos_kernel_ref(x, x) + sigma * torch.eye(n, dtype=torch.float64)).float()
    F = torch.randn(3, n, m, generator=torch.Generator().manual_seed(1))
    return K, F


def solve_errors(X, K, F, ref):
    """(forward, backward) error of a solution X of the fp32-stored system, both in fp64: max|X - ref| / max|ref| and the normwise
    backward error |K X - F|_F / (|K|_F |X|_F)."""
    X, K, F = X.detach().cpu().double(), K.detach().cpu().double(), F.detach().cpu().double()
    fwd = float((X - ref).abs().max() / ref.abs().max())
    bwd = float(torch.linalg.norm(K @ X - F) / (torch.linalg.norm(K) * torch.linalg.norm(X)))
    return fwd, bwd


def fp32_solve(K, F):
    """The plain fp32 reference of spd_solve: LAPACK Cholesky factorisation + solve in fp32 on the CPU, one thread."""
    return single_thread(lambda: torch.cholesky_solve(F.float().cpu(), torch.linalg.cholesky(K.float().cpu())))


def well_conditioned_system(B, n, m, seed, D=32):
    """The recipe of the solver tests in test_gpu_ops.py: random unit vectors, K = exp((<x,x> - 1)/0.2) + 0.1 I, F ~ N(0,1); fp32."""
    g = torch.Generator().manual_seed(seed)
    x = torch.nn.functional.normalize(torch.randn(B, n, D, generator=g), dim=-1)
    K = torch.exp((x @ x.transpose(1, 2) - 1) / 0.2) + 0.1 * torch.eye(n)
    return K, torch.randn(B, n, m, generator=g)


def state_before_step(K, F, j, nb=NB):
    """The augmented matrix [K | F] in fp64 as it stands when the step at block row j begins: the steps before it applied in full
    (chol_step_ref chained), rows above j left as they were.  Returns A (B, n, n+m) fp64."""
    n, m = K.shape[1], F.shape[2]
    A = torch.cat((K, F), dim=2).double().clone()
    for (a, e) in blocks(n, nb):
        if a >= j:
            break
        W = torch.linalg.inv(torch.linalg.cholesky(A[:, a:e, a:e]))
        _, trailing, _, _ = chol_step_ref(A, n, n + m, a, e - a, W)
        A[:, e:, e:] = trailing
    return A


def blocked_solve_ref(K, F, nb=NB):
    """The whole blocked solve out of the step references: chol_step_ref over all blocks, then subst_step_ref backwards."""
    B, n, m = K.shape[0], K.shape[1], F.shape[2]
    A = torch.cat((K, F), dim=2).double().clone()
    Lfull = torch.zeros(B, n, n, dtype=torch.float64)
    Y = torch.zeros(B, n, m, dtype=torch.float64)
    Wb = []
    Lkk = torch.linalg.cholesky(A[:, :min(nb, n), :min(nb, n)])
    W = torch.linalg.inv(Lkk)
    for (j, e) in blocks(n, nb):
        R, trailing, Ln, Wn = chol_step_ref(A, n, n + m, j, e - j, W)
        Lfull[:, j:e, j:e] = Lkk
        Lfull[:, e:, j:e] = R[:, :, :n - e].transpose(1, 2)
        Y[:, j:e] = R[:, :, n - e:]
        A[:, e:, e:] = trailing
        Wb.append(W)
        Lkk, W = Ln, Wn
    X = torch.zeros(B, n, m, dtype=torch.float64)
    T = Y
    for s in range(len(Wb) - 1, -1, -1):
        Xs, T = subst_step_ref(-1, Lfull, Wb, T, s, nb)
        X[:, s * nb:s * nb + Xs.shape[1]] = Xs
    return X, Lfull, Wb, Y


# ---- error bounds of the fp32 kernels against these references ------------------------------------------------------------------
# Everything the solver kernels do apart from the 64 x 64 factorisation is a product of fp32 numbers accumulated in fp32, for which
# the classical bound holds whatever the order of summation and with or without FMA (Higham, Accuracy and Stability, 3.1):
#   |fl(sum_{i<k} a_i b_i) - sum a_i b_i| <= gamma_k sum |a_i||b_i|,   gamma_k = k u / (1 - k u),   u = 2^-24.
# The bounds below are these, elementwise, with k + 2 for gamma_k (covers 1 / (1 - k u) and the rounding of the stored result).
def product_bound(absA, absB, k):
    """Elementwise bound on the fp32 evaluation of A @ B (inner dimension k) given |A|, |B| in fp64."""
    return (k + 2) * U32 * (absA @ absB)


def step_bounds(A, n, ncols, j, nb, W):
    """Elementwise bounds (R, trailing) for roma_chol_step on the fp32-stored A, W: R = W A is one product; the update
    A - R^T R uses the COMPUTED R (error dR <= bR) in a second product and one subtraction:
      |dT| <= u |A| + gamma |R|^T |R| + |dR|^T |R| + |R|^T |dR|  <=  u |A| + 3 (nb + 2) u P^T P,   P = |W| |A[j:e, e:]| >= |R|, bR."""
    e = j + nb
    A = A.double()
    P = W.double().abs() @ A[:, j:e, e:ncols].abs()
    bR = (nb + 2) * U32 * P
    bT = U32 * A[:, e:n, e:ncols].abs() + 3 * (nb + 2) * U32 * (P[:, :, :n - e].transpose(1, 2) @ P)
    return bR, bT


def factor_bounds(Ablk, dA=None):
    """Bounds on max|L - Lref| and max|W - inv(Lref)| for the fp32 factorisation of a w x w block (lower triangle of Ablk, fp64),
    per batch item.  The computed factor is the exact factor of Ablk + E with |E| <= 4 (w + 2) u |L||L|^T (Higham Thm 10.3 has
    gamma_{w+1}; the 4 covers the kernel's 1-ulp reciprocal, the product with it and the Newton-corrected 1/sqrt in each of the w
    rank-1 steps) + dA, the error the block arrived with.  First-order perturbation of the Cholesky factor (Sun 1991; Higham Thm
    10.8):  |dL|_F <= cond_2(A) / sqrt(2) * |E|_F / |L|_2.   For the inverse, d(L^-1) = -L^-1 dL L^-1 plus the substitution's own
    error gamma cond(L) |L^-1|:  |dW| <= |W|_2^2 |dL|_F + 4 (w + 2) u cond_2(L) |W|_2."""
    Ablk = Ablk.double()
    w = Ablk.shape[-1]
    L = torch.linalg.cholesky(Ablk)
    Wi = torch.linalg.inv(L)
    E = 4 * (w + 2) * U32 * (L.abs() @ L.abs().transpose(1, 2))
    if dA is not None:
        E = E + dA
    nL, nW = torch.linalg.matrix_norm(L, 2), torch.linalg.matrix_norm(Wi, 2)
    tolL = (nL * nW) ** 2 / 2 ** 0.5 * torch.linalg.matrix_norm(E) / nL
    tolW = nW ** 2 * tolL + 4 * (w + 2) * U32 * (nL * nW) * nW
    return L, Wi, tolL, tolW
